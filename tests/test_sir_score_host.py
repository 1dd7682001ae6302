"""No GPU: the Monte-Carlo source scores -- the two entries' binding against the header, the size query and the entry without a
handle, every ValueError of gnode.ode_nn.source_scores_mc with the library out of reach, and SirSourceScores' two tables on a
hand-made histogram."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sir_score_model as Q
from sir_host_cases import N, RING, Reached, lib, no_library, shared_refusals  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"gnode_sir_sweep_scores_workspace_bytes": 6, "gnode_sir_mc_philox_sweep_scores": 24}


# --------------------------------------------------------------------------------------------------------------- the ABI
def test_the_two_entries_are_bound_with_the_headers_arity():
    from gnode import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnode.h")).read(), flags=re.S)
    protos = {name: params for _, name, params in re.findall(r"^(size_t|int)\s*(gnode_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M)}
    for name, arity in ARITY.items():
        assert name in _lib.EXPORTS and protos[name].count(",") + 1 == arity == len(_lib.ABI[name][1]), name
    assert len(_lib.ABI["gnode_sir_mc_philox_sweep"][1]) == 21      # the sweep's entry is what it was


def test_the_version_stays_and_the_entry_refuses_without_a_handle(lib):
    assert lib.gnode_version() == 226                               # a stale library is known by the missing symbol
    assert lib.gnode_sir_sweep_scores_workspace_bytes(None, 10, 2, 12, 5, 3) == 0
    init = np.ascontiguousarray(np.tile([1.0, 0.0, 0.0], (4, 1)))
    cand, phase, obs = np.zeros(1, np.int32), np.zeros(3, np.int32), np.zeros((1, 4), np.int8)
    w, gam = np.zeros((1, 6)), np.zeros((1, 4))
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    status = lib.gnode_sir_mc_philox_sweep_scores(None, hp(init), hp(cand), None, 1, 0, hp(phase), 1, 3, hp(w), hp(gam), hp(obs), 1, 0, 64, 4, 0, 3,
                                                  C.c_uint64(1), None, None, 0, None, 0)
    assert status == -1 and "gnode_sir_mc_philox_sweep_scores" in lib.gnode_last_error().decode()


# --------------------------------------------------------------------------------------------------------------- refusals
def test_source_scores_mc_refuses_before_the_library(no_library):
    import torch
    from gnode.ode_nn import rate_schedule, source_scores_mc
    short = rate_schedule([0.2, 0.4], steps=[0, 0, 0, 1, 1, 0])     # names 6 entries: calendar steps up to 5
    snap = [0, 1, 2, -1, 0, 0]
    good = dict(graph=RING, obs=snap, beta=0.3, gamma=0.2, sims=10, maxTime=4, candidates=[0, 3, -1])
    bad = [
        dict(obs=snap[:5]), dict(obs=[snap[:5]]), dict(obs=[0, 1, 3, -1, 0, 0]), dict(obs=[0, 1, -2, -1, 0, 0]), dict(obs=[-1] * N),
        dict(obs=[snap, [-1] * N]), dict(obs=np.asarray(snap, float)), dict(obs=np.zeros((0, N), np.int8)), dict(obs=np.zeros((2, 1, N), np.int8)),
        dict(obs=torch.tensor(snap, dtype=torch.float32)), dict(obs=None),
        dict(measure="cosine"), dict(measure=0), dict(bins=0), dict(bins=4097), dict(bins=2.5), dict(bins="many"),
        dict(bins=4096, candidates=list(range(N)) * 5000, maxTime=20),            # 30 000 x 20 x 4097 cells >= 2^31
        dict(hist=torch.zeros((1, 3, 4, 65), dtype=torch.int32)), dict(hist=torch.zeros((3, 4, 65), dtype=torch.int64)), dict(hist=np.zeros((1, 3, 4, 65))),
        dict(hist=torch.zeros((1, 3, 4, 64), dtype=torch.int64)), dict(obs=[snap, snap], hist=torch.zeros((1, 3, 4, 65), dtype=torch.int64)),
        *shared_refusals(),                                         # what outbreak_sizes_mc refuses, through the shared checks
    ]
    for change in bad:
        with pytest.raises(ValueError):
            source_scores_mc(**dict(good, **change))
    with pytest.raises(TypeError):
        source_scores_mc(**dict(good, action="immunise"))           # the action is fixed: a source is seeded
    for ok in (good, dict(good, obs=[snap, snap]), dict(good, obs=np.asarray([snap] * 17, np.int8)), dict(good, obs=torch.tensor(snap, dtype=torch.int8)),
               dict(good, obs=np.asarray(snap, np.int64)), dict(good, measure="match", bins=7), dict(good, bins=4096), dict(good, shifts=[0, 2, 5]),
               dict(good, gamma=short, shifts=[0, 2, 0]), dict(good, candidates=None), dict(good, start=[1]), dict(good, start=None), dict(good, sims=0),
               dict(good, hist=torch.zeros((1, 3, 4, 65), dtype=torch.int64)), dict(good, obs=[snap] * 17, hist=torch.zeros((17, 3, 4, 65), dtype=torch.int64))):
        with pytest.raises(Reached):                                # everything was in order: the next thing is the library
            source_scores_mc(**ok)


def test_outbreak_sizes_mc_still_refuses_through_the_shared_checks(no_library):
    from gnode.ode_nn import outbreak_sizes_mc
    for change in (dict(candidates=[0, N]), dict(shifts=[0, -1, 2]), dict(action="cure"), dict(action="immunise", start=None), dict(sims=-1)):
        with pytest.raises(ValueError):
            outbreak_sizes_mc(**dict(dict(graph=RING, beta=0.3, gamma=0.2, sims=10, maxTime=4, candidates=[0, 3, -1], start=[1]), **change))


# ------------------------------------------------------------------------------------------------------------ the tables
def test_scores_and_exact_on_a_hand_made_histogram():
    import torch
    from gnode.dmp import rank_sources, source_rank_of
    from gnode.ode_nn import SirSourceScores
    rng = np.random.default_rng(5)
    O, Cn, T, bins, sims = 2, 4, 3, 7, 50
    h = rng.multinomial(sims, np.full(bins + 1, 1.0 / (bins + 1)), size=(O, Cn, T)).astype(np.int64)
    h[0, 1, 2] = 0; h[0, 1, 2, bins] = sims                         # candidate 1 agrees completely at t = 2, in every trajectory
    h[1, 3, 0] = 0; h[1, 3, 0, 0] = sims                            # candidate 3 at t = 0: no similarity at all
    h[1, 2, 1, bins] = 0
    r = SirSourceScores(torch.from_numpy(h), sims, bins, False)
    assert r.exact().dtype == torch.float64 and torch.equal(r.exact(), torch.from_numpy(h[..., bins] / sims))
    for width in (0.25, 1.0, 0.05):
        want = np.log(np.maximum(1e-30, (h * np.exp(-(1.0 - np.arange(bins + 1) / bins) ** 2 / width ** 2)).sum(-1) / sims))
        got = r.scores(width=width)
        assert got.dtype == torch.float64 and tuple(got.shape) == (O, Cn, T) and np.allclose(got.numpy(), want, rtol=1e-13, atol=0)
        assert np.allclose(got.numpy(), Q.kernel_scores(h.astype(np.uint64), sims, width), rtol=1e-13, atol=0)
    assert r.scores()[0, 1, 2] == 0.0                               # the top bin is phi = 1 exactly: weight 1
    assert np.isclose(float(r.scores(width=0.5)[1, 3, 0]), -4.0)    # a bin at its lower edge: phi = 0, exp(-1 / 0.25)
    assert float(r.scores(width=0.01, floor=1e-12)[1, 3, 0]) == np.log(1e-12)
    with pytest.raises(ValueError):
        r.scores(width=0.0)
    one = SirSourceScores(torch.from_numpy(h[:1]), sims, bins, True)          # one snapshot given as [n]: [C, T] tables
    assert tuple(one.scores().shape) == (Cn, T) == tuple(one.exact().shape) and torch.equal(one.scores(), r.scores()[0])
    ranked = rank_sources(one.scores(), [10, 11, 12, 13])
    assert ranked[0] == (11, 2, 0.0) and len(ranked) == Cn
    loglik = torch.log(torch.clamp(one.exact(), min=1e-30))         # the exact-match frequency, floored, ranks the same way
    assert rank_sources(loglik, [10, 11, 12, 13])[0] == (11, 2, 0.0)
    assert source_rank_of(r.scores(), [10, 11, 12, 13], [11, 13]).tolist()[0] == 0
    assert float(torch.log(torch.clamp(r.exact(), min=1e-30))[1, 2, 1]) == np.log(1e-30)
