"""No GPU: the Monte-Carlo nowcast and forecast from timed evidence -- the two entries' binding against the header, the size query
and the entry without a handle, every ValueError of gnode.ode_nn.posterior_states_mc with the library out of reach, and what
SirPosterior makes of the integers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sir_host_cases import N, RING, Reached, _obs, lib, no_library, shared_refusals  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"gnode_sir_sweep_posterior_workspace_bytes": 8, "gnode_sir_mc_philox_sweep_posterior": 30}


# --------------------------------------------------------------------------------------------------------------- the ABI
def test_the_two_entries_are_bound_with_the_headers_arity():
    from gnode import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnode.h")).read(), flags=re.S)
    protos = {name: params for _, name, params in re.findall(r"^(size_t|int)\s*(gnode_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M)}
    for name, arity in ARITY.items():
        assert name in _lib.EXPORTS and protos[name].count(",") + 1 == arity == len(_lib.ABI[name][1]), name
    assert len(_lib.ABI["gnode_sir_mc_philox_sweep_timed"][1]) == 27 and len(_lib.ABI["gnode_sir_sweep_timed_workspace_bytes"][1]) == 7   # what they were
    # the timed entry's arguments with bins replaced by (now, horizons, H) and hist by (counts, accepted)
    timed, post = _lib.ABI["gnode_sir_mc_philox_sweep_timed"][1], _lib.ABI["gnode_sir_mc_philox_sweep_posterior"][1]
    assert post[:17] == timed[:17] and post[17:20] == [C.c_int32, C.c_void_p, C.c_int32] and post[20:24] == timed[18:22]
    assert post[24:26] == [C.c_void_p] * 2 and post[26:] == timed[23:]


def test_the_version_stays_and_the_entry_refuses_without_a_handle(lib):
    assert lib.gnode_version() == 226                               # a stale library is known by the missing symbol
    assert lib.gnode_sir_sweep_posterior_workspace_bytes(None, 10, 2, 12, 5, 3, 9, 2) == 0
    init = np.ascontiguousarray(np.tile([1.0, 0.0, 0.0], (4, 1)))
    cand, phase, rec = np.zeros(1, np.int32), np.zeros(3, np.int32), np.zeros(1, np.int32)
    w, gam = np.zeros((1, 6)), np.zeros((1, 4))
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    status = lib.gnode_sir_mc_philox_sweep_posterior(None, hp(init), hp(cand), None, 1, 0, hp(phase), 1, 3, hp(w), hp(gam), hp(rec), hp(rec), hp(rec), hp(rec),
                                                     1, 1, 1, hp(rec), 1, 4, 0, 3, C.c_uint64(1), None, None, None, 0, None, 0)
    assert status == -1 and "gnode_sir_mc_philox_sweep_posterior" in lib.gnode_last_error().decode()


# --------------------------------------------------------------------------------------------------------------- refusals
def test_posterior_states_mc_refuses_before_the_library(no_library):
    import torch
    from gnode.dmp import timed_observations
    from gnode.ode_nn import posterior_states_mc, rate_schedule
    short = rate_schedule([0.2, 0.4], steps=[0, 0, 0, 1, 1, 0])     # names 6 entries: calendar steps up to 5
    ev = timed_observations(N, [0, 2, 2, 5], [0, -1, 0, -3], [1, 3, 2, 0])
    row = [0, 1, 4, -1, 3, 0]
    good = dict(graph=RING, observations=ev, beta=0.3, gamma=0.2, sims=10, maxTime=4, now=1, candidates=[0, 3, -1])
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64)      # noqa: E731
    bad = [
        dict(now=-1), dict(now=4), dict(now=1.5), dict(now="today"), dict(now=None), dict(now=True),
        dict(horizons=[]), dict(horizons=[-1]), dict(horizons=[0, 0]), dict(horizons=[1, 0]), dict(horizons=[0, 3]), dict(horizons=[3]),
        dict(horizons=[0.5]), dict(horizons="soon"), dict(horizons=None), dict(horizons=[[0, 1]]), dict(now=3, horizons=1),
        dict(maxTime=40, horizons=list(range(33))),
        dict(observations=None), dict(observations=[]), dict(observations=np.asarray(row, np.int8)), dict(observations=[ev, row]), dict(observations=7),
        dict(observations=_obs([row[:5]], [0], n=5)), dict(observations=_obs([row], [0, -1])), dict(observations=_obs([row], [1])),
        dict(observations=_obs([[0, 1, 5, -1, 3, 0]], [0])), dict(observations=_obs([[-1] * N], [0])), dict(observations=[ev, _obs([[-1] * N], [0])]),
        dict(counts=torch.zeros((1, 1, 2, N), dtype=torch.int32)), dict(counts=i64(1, 2, N)), dict(counts=np.zeros((1, 1, 2, N))), dict(counts=i64(1, 1, 2, N + 1)),
        dict(counts=i64(1, 2, 2, N)), dict(accepted=i64(1, 2)), dict(accepted=i64(3)), dict(accepted=torch.zeros((1, 3), dtype=torch.int32)),
        dict(observations=[ev, ev], counts=i64(1, 1, 2, N)), dict(observations=[ev, ev], accepted=i64(1, 3)),
        *shared_refusals(),                                         # what outbreak_sizes_mc refuses, through the shared checks
    ]
    for change in bad:
        with pytest.raises(ValueError):
            posterior_states_mc(**dict(good, **change))
    with pytest.raises(ValueError, match=r"horizons\[1\] = 3"):
        posterior_states_mc(**dict(good, horizons=[0, 3]))
    with pytest.raises(ValueError, match=r"horizons\[2\] = 1"):
        posterior_states_mc(**dict(good, horizons=[0, 1, 1]))
    with pytest.raises(TypeError):
        posterior_states_mc(**dict(good, action="immunise"))        # the action is fixed: a source is seeded
    with pytest.raises(TypeError):
        posterior_states_mc(**dict(good, bins=4))                   # and nothing is binned
    for ok in (good, dict(good, observations=[ev, ev]), dict(good, observations=[ev] * 17), dict(good, observations=(ev,)),
               dict(good, now=0), dict(good, now=3), dict(good, now=0, horizons=[0, 1, 2, 3]), dict(good, horizons=(0, 2)), dict(good, horizons=2),
               dict(good, horizons=np.asarray([1, 2])), dict(good, horizons=[1.0]), dict(good, maxTime=5000, now=2500, horizons=range(0, 64, 2)),
               dict(good, observations=[ev] * 40, maxTime=200, now=100), dict(good, observations=_obs(np.zeros((1000, N), np.int8), -np.arange(1000))),
               dict(good, shifts=[0, 2, 5]), dict(good, gamma=short, shifts=[0, 2, 0]), dict(good, candidates=None), dict(good, start=[1]),
               dict(good, start=None), dict(good, sims=0), dict(good, counts=i64(1, 1, 2, N), accepted=i64(1, 3)), dict(good, accepted=i64(1, 3)),
               dict(good, observations=[ev] * 17, horizons=[0, 1], counts=i64(17, 2, 2, N), accepted=i64(17, 3))):
        with pytest.raises(Reached):                                # everything was in order: the next thing is the library
            posterior_states_mc(**ok)


# -------------------------------------------------------------------------------------------------------------- the result
def test_sir_posterior_reads_the_integers():
    import torch
    from gnode.ode_nn import SirPosterior
    counts = torch.zeros((2, 2, 2, 3), dtype=torch.int64)
    counts[0, 0, 0] = torch.tensor([4, 0, 1]); counts[0, 0, 1] = torch.tensor([1, 0, 0]); counts[0, 1, 0] = torch.tensor([2, 1, 1]); counts[0, 1, 1] = torch.tensor([3, 0, 0])
    accepted = torch.tensor([[3, 2, 0], [0, 0, 0]])
    r = SirPosterior(counts, accepted, 10, 4, (0, 2), False)
    assert r.accepted_total().tolist() == [5, 0] and r.accepted_total().dtype == torch.int64
    src = r.source()
    assert src.dtype == torch.float64 and tuple(src.shape) == (2, 3) and src[0].tolist() == [0.6, 0.4, 0.0] and bool(torch.isnan(src[1]).all())
    m = r.marginals()
    assert m.dtype == torch.float64 and tuple(m.shape) == (2, 2, 3, 3) and bool(torch.isnan(m[1]).all())
    assert m[0, 0].tolist() == [[0.0, 0.8, 0.2], [1.0, 0.0, 0.0], [0.8, 0.2, 0.0]] and m[0, 1].tolist() == [[0.0, 0.4, 0.6], [0.8, 0.2, 0.0], [0.8, 0.2, 0.0]]
    assert torch.allclose(m[0].sum(-1), torch.ones((2, 3), dtype=torch.float64), rtol=0, atol=1e-15)
    one = SirPosterior(counts[:1], accepted[:1], 10, 4, (0, 2), True)
    assert tuple(one.marginals().shape) == (2, 3, 3) and tuple(one.source().shape) == (3,) and int(one.accepted_total()) == 5
    assert torch.equal(one.marginals(), m[0])
