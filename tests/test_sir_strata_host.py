"""No GPU: the Monte-Carlo nowcast from evidence that may be wrong -- the entry's binding against the header, the entry without a
handle, every ValueError of gnode.ode_nn.posterior_strata_mc with the library out of reach, and what SirPosteriorStrata makes of
the integers."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from sir_host_cases import N, RING, Reached, _obs, lib, no_library, shared_refusals  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "gnode_sir_mc_philox_sweep_posterior_strata"


# --------------------------------------------------------------------------------------------------------------- the ABI
def test_the_entry_is_bound_with_the_headers_arity():
    from gnode import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnode.h")).read(), flags=re.S)
    protos = {name: params for _, name, params in re.findall(r"^(size_t|int)\s*(gnode_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M)}
    assert ENTRY in _lib.EXPORTS and protos[ENTRY].count(",") + 1 == 31 == len(_lib.ABI[ENTRY][1])
    # the posterior entry's arguments with one int32, mismatches, after H; the posterior's own stay what they were
    post, strata = _lib.ABI["gnode_sir_mc_philox_sweep_posterior"][1], _lib.ABI[ENTRY][1]
    assert len(post) == 30 and strata == post[:20] + [C.c_int32] + post[20:] and _lib.ABI[ENTRY][0] == _lib.ABI["gnode_sir_mc_philox_sweep_posterior"][0]
    names = [p.split()[-1].lstrip("*") for p in protos[ENTRY].split(",")]
    assert names[19:22] == ["H", "mismatches", "sims"] and names[:20] + names[21:] == [p.split()[-1].lstrip("*") for p in protos["gnode_sir_mc_philox_sweep_posterior"].split(",")]
    assert not any("strata_workspace" in name for name in _lib.EXPORTS)      # the workspace is the posterior's: no size query of its own


def test_the_version_stays_and_the_entry_refuses_without_a_handle(lib):
    assert lib.gnode_version() == 226                               # a stale library is known by the missing symbol
    init = np.ascontiguousarray(np.tile([1.0, 0.0, 0.0], (4, 1)))
    cand, phase, rec = np.zeros(1, np.int32), np.zeros(3, np.int32), np.zeros(1, np.int32)
    w, gam = np.zeros((1, 6)), np.zeros((1, 4))
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    status = getattr(lib, ENTRY)(None, hp(init), hp(cand), None, 1, 0, hp(phase), 1, 3, hp(w), hp(gam), hp(rec), hp(rec), hp(rec), hp(rec),
                                 1, 1, 1, hp(rec), 1, 1, 4, 0, 3, C.c_uint64(1), None, None, None, 0, None, 0)
    assert status == -1 and ENTRY in lib.gnode_last_error().decode()


# --------------------------------------------------------------------------------------------------------------- refusals
def test_posterior_strata_mc_refuses_before_the_library(no_library):
    import torch
    from gnode.dmp import timed_observations
    from gnode.ode_nn import posterior_strata_mc, rate_schedule
    short = rate_schedule([0.2, 0.4], steps=[0, 0, 0, 1, 1, 0])     # names 6 entries: calendar steps up to 5
    ev = timed_observations(N, [0, 2, 2, 5], [0, -1, 0, -3], [1, 3, 2, 0])
    row = [0, 1, 4, -1, 3, 0]
    good = dict(graph=RING, observations=ev, beta=0.3, gamma=0.2, sims=10, maxTime=4, now=1, candidates=[0, 3, -1])   # mismatches = 1: D = 2
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64)      # noqa: E731
    bad = [
        dict(mismatches=-1), dict(mismatches=8), dict(mismatches=1.5), dict(mismatches=True), dict(mismatches=None), dict(mismatches="two"),
        dict(mismatches=[1]), dict(mismatches=float("nan")), dict(mismatches=2**31),
        dict(now=-1), dict(now=4), dict(now=1.5), dict(now="today"), dict(now=None), dict(now=True),
        dict(horizons=[]), dict(horizons=[-1]), dict(horizons=[0, 0]), dict(horizons=[1, 0]), dict(horizons=[0, 3]), dict(horizons=[3]),
        dict(horizons=[0.5]), dict(horizons="soon"), dict(horizons=None), dict(horizons=[[0, 1]]), dict(now=3, horizons=1),
        dict(maxTime=40, horizons=list(range(33))),
        dict(observations=None), dict(observations=[]), dict(observations=np.asarray(row, np.int8)), dict(observations=[ev, row]), dict(observations=7),
        dict(observations=_obs([row[:5]], [0], n=5)), dict(observations=_obs([row], [0, -1])), dict(observations=_obs([row], [1])),
        dict(observations=_obs([[0, 1, 5, -1, 3, 0]], [0])), dict(observations=_obs([[-1] * N], [0])), dict(observations=[ev, _obs([[-1] * N], [0])]),
        # counts [O, D, H, 2, n] and accepted [O, C, D]: the posterior's shapes are wrong here, and so is another D
        dict(counts=torch.zeros((1, 2, 1, 2, N), dtype=torch.int32)), dict(counts=i64(1, 1, 2, N)), dict(counts=np.zeros((1, 2, 1, 2, N))),
        dict(counts=i64(1, 2, 1, 2, N + 1)), dict(counts=i64(1, 2, 2, 2, N)), dict(counts=i64(1, 3, 1, 2, N)), dict(counts=i64(1, 1, 1, 2, N)),
        dict(counts=i64(1, 2, 1, 2, 2 * N)[..., ::2]), dict(mismatches=2, counts=i64(1, 2, 1, 2, N)),
        dict(accepted=i64(1, 3)), dict(accepted=i64(1, 3, 3)), dict(accepted=i64(1, 2, 2)), dict(accepted=i64(3, 2)), dict(accepted=i64(1, 2, 3).transpose(1, 2)),
        dict(accepted=torch.zeros((1, 3, 2), dtype=torch.int32)), dict(accepted=np.zeros((1, 3, 2), np.int64)), dict(mismatches=0, accepted=i64(1, 3, 2)),
        dict(observations=[ev, ev], counts=i64(1, 2, 1, 2, N)), dict(observations=[ev, ev], accepted=i64(1, 3, 2)),
        *shared_refusals(),                                         # what outbreak_sizes_mc refuses, through the shared checks
    ]
    for change in bad:
        with pytest.raises(ValueError):
            posterior_strata_mc(**dict(good, **change))
    with pytest.raises(ValueError, match=r"mismatches = 8 is not in \[0, 7\]"):
        posterior_strata_mc(**dict(good, mismatches=8))
    with pytest.raises(ValueError, match=r"mismatches must be a whole number >= 0, got -1"):
        posterior_strata_mc(**dict(good, mismatches=-1))
    with pytest.raises(ValueError, match=r"horizons\[1\] = 3"):
        posterior_strata_mc(**dict(good, horizons=[0, 3]))
    with pytest.raises(ValueError, match=r"accepted must be a contiguous int64 tensor of shape \(1, 3, 2\)"):
        posterior_strata_mc(**dict(good, accepted=i64(1, 3)))
    with pytest.raises(ValueError, match=r"counts must be a contiguous int64 tensor of shape \(1, 2, 1, 2, 6\)"):
        posterior_strata_mc(**dict(good, counts=i64(1, 1, 2, N)))
    with pytest.raises(TypeError):
        posterior_strata_mc(**dict(good, action="immunise"))        # the action is fixed: a source is seeded
    for ok in (good, dict(good, mismatches=0), dict(good, mismatches=7), dict(good, mismatches=2.0), dict(good, mismatches=np.int32(3)),
               dict(good, observations=[ev, ev]), dict(good, observations=[ev] * 17), dict(good, observations=(ev,)),
               dict(good, now=0), dict(good, now=3), dict(good, now=0, horizons=[0, 1, 2, 3]), dict(good, horizons=(0, 2)), dict(good, horizons=2),
               dict(good, maxTime=5000, now=2500, horizons=range(0, 64, 2), mismatches=7),
               dict(good, observations=_obs(np.zeros((1000, N), np.int8), -np.arange(1000))),
               dict(good, shifts=[0, 2, 5]), dict(good, gamma=short, shifts=[0, 2, 0]), dict(good, candidates=None), dict(good, start=[1]),
               dict(good, sims=0), dict(good, counts=i64(1, 2, 1, 2, N), accepted=i64(1, 3, 2)), dict(good, accepted=i64(1, 3, 2)),
               dict(good, mismatches=0, counts=i64(1, 1, 1, 2, N), accepted=i64(1, 3, 1)),
               dict(good, observations=[ev] * 17, horizons=[0, 1], mismatches=4, counts=i64(17, 5, 2, 2, N), accepted=i64(17, 3, 5))):
        with pytest.raises(Reached):                                # everything was in order: the next thing is the library
            posterior_strata_mc(**ok)


# -------------------------------------------------------------------------------------------------------------- the result
def _result(squeezed=False):
    """two sets, D = 3, H = 2, n = 3, C = 2: set 0 with 2 records (complete at M = 2), set 1 with 5 and nothing accepted"""
    import torch
    from gnode.ode_nn import SirPosteriorStrata
    counts = torch.zeros((2, 3, 2, 2, 3), dtype=torch.int64)
    counts[0, 0, 0, 0] = torch.tensor([4, 0, 1]); counts[0, 0, 0, 1] = torch.tensor([1, 0, 0])       # stratum 0: 5 accepted
    counts[0, 0, 1, 0] = torch.tensor([2, 1, 1]); counts[0, 0, 1, 1] = torch.tensor([3, 0, 0])
    counts[0, 1, 0, 0] = torch.tensor([10, 5, 0]); counts[0, 1, 0, 1] = torch.tensor([10, 0, 0])     # stratum 1: 20
    counts[0, 1, 1, 0] = torch.tensor([0, 10, 0]); counts[0, 1, 1, 1] = torch.tensor([20, 0, 0])
    counts[0, 2, 0, 0] = torch.tensor([0, 0, 75]); counts[0, 2, 1, 1] = torch.tensor([0, 0, 75])     # stratum 2: 75
    accepted = torch.tensor([[[3, 12, 35], [2, 8, 40]], [[0, 0, 0], [0, 0, 0]]])
    if squeezed:
        return SirPosteriorStrata(counts[:1], accepted[:1], 50, 4, (0, 2), (2,), True)
    return SirPosteriorStrata(counts, accepted, 50, 4, (0, 2), (2, 5), False)


def test_the_weights():
    import torch
    r = _result()
    assert r.mismatches == 2
    assert r.weights(0).tolist() == [1.0, 0.0, 0.0] and r.weights(0.0).dtype == torch.float64
    assert r.weights(0.5).tolist() == [1.0, 1.0, 1.0]
    w = r.weights(0.1).tolist()
    assert w[0] == 1.0 and math.isclose(w[1], 1.0 / 9.0, rel_tol=1e-15) and math.isclose(w[2], 1.0 / 81.0, rel_tol=1e-15)
    for bad in (-0.1, 1.0, 1.5, float("nan"), None, "0.1", True, [0.1]):
        with pytest.raises(ValueError):
            r.weights(bad)


def test_exactly_one_of_error_and_weights():
    r = _result()
    for method in (r.source, r.marginals, r.ess):
        with pytest.raises(ValueError, match="exactly one"):
            method()
        with pytest.raises(ValueError, match="exactly one"):
            method(error=0.1, weights=[1, 1, 1])
        for bad in ([1, 1], [1, 1, 1, 1], [0, 0, 0], [1, -1, 1], [1, float("inf"), 0], [1, float("nan"), 0], "abc", [[1, 1, 1]], 1.0):
            with pytest.raises(ValueError, match="weights must be 3 finite numbers"):
                method(weights=bad)
        with pytest.raises(ValueError):
            method(error=1.0)
        assert method(0.1).dtype == method(weights=(1, 0.5, 0)).dtype        # error is the first argument


def test_nan_where_nothing_is_accepted_and_the_marginals_sum_to_one():
    import torch
    r = _result()
    for kw in (dict(error=0.0), dict(error=0.1), dict(error=0.5), dict(weights=[1, 1, 1]), dict(weights=[0, 0, 2.5])):
        m, s, e = r.marginals(**kw), r.source(**kw), r.ess(**kw)
        assert m.dtype == s.dtype == e.dtype == torch.float64 and tuple(m.shape) == (2, 2, 3, 3) and tuple(s.shape) == (2, 2) and tuple(e.shape) == (2,)
        assert bool(torch.isnan(m[1]).all()) and bool(torch.isnan(s[1]).all()) and bool(torch.isnan(e[1]))
        assert torch.allclose(m[0].sum(-1), torch.ones((2, 3), dtype=torch.float64), rtol=0, atol=1e-15) and bool((m[0] >= 0).all())
        assert math.isclose(float(s[0].sum()), 1.0, rel_tol=0, abs_tol=1e-15)
    # error 0 is the exact-match posterior: stratum 0 alone
    m = r.marginals(error=0)
    assert m[0, 0].tolist() == [[0.0, 0.8, 0.2], [1.0, 0.0, 0.0], [0.8, 0.2, 0.0]] and m[0, 1].tolist() == [[0.0, 0.4, 0.6], [0.8, 0.2, 0.0], [0.8, 0.2, 0.0]]
    assert r.source(error=0)[0].tolist() == [0.6, 0.4] and torch.equal(m[0], r.exact().marginals()[0])
    # flat weights: all 100 accepted trajectories count alike
    m = r.marginals(weights=[1, 1, 1])
    assert m[0, 0].tolist() == [[0.75, 0.14, 0.11], [0.95, 0.05, 0.0], [0.24, 0.76, 0.0]] and r.source(weights=[2, 2, 2])[0].tolist() == [0.5, 0.5]
    # weights (1, 1/2, 0): total 5 + 10 = 15; node 0 at h = 0: I = 4 + 5, R = 1 + 5
    m = r.marginals(weights=[1, 0.5, 0])
    assert torch.allclose(m[0, 0, 0], torch.tensor([0.0, 9.0, 6.0], dtype=torch.float64) / 15.0, rtol=1e-15, atol=0)
    assert torch.allclose(r.source(weights=[1, 0.5, 0])[0], torch.tensor([9.0, 6.0], dtype=torch.float64) / 15.0, rtol=1e-15, atol=0)
    # error 0.1: w = (1, 1/9, 1/81)
    tot = 5 + 20 / 9 + 75 / 81
    assert math.isclose(float(r.marginals(error=0.1)[0, 0, 2, 1]), (1 + 75 / 81) / tot, rel_tol=1e-14)
    assert math.isclose(float(r.source(error=0.1)[0, 0]), (3 + 12 / 9 + 35 / 81) / tot, rel_tol=1e-14)


def test_by_stratum_ess_complete_and_exact():
    import torch
    r = _result()
    by = r.by_stratum()
    assert by.dtype == torch.int64 and by.tolist() == [[5, 20, 75], [0, 0, 0]]
    assert float(r.ess(error=0)[0]) == 5.0 and float(r.ess(weights=[1, 1, 1])[0]) == 100.0 and float(r.ess(weights=[3, 3, 3])[0]) == 100.0
    assert math.isclose(float(r.ess(weights=[1, 0.5, 0])[0]), 15.0 ** 2 / (5 + 20 / 4), rel_tol=1e-15)
    assert math.isclose(float(r.ess(error=0.1)[0]), (5 + 20 / 9 + 75 / 81) ** 2 / (5 + 20 / 81 + 75 / 6561), rel_tol=1e-14)
    assert float(r.ess(error=0)[0]) < float(r.ess(error=0.05)[0]) < float(r.ess(error=0.3)[0]) < 100.0
    assert r.complete().dtype == torch.bool and r.complete().tolist() == [True, False]
    x = r.exact()
    assert type(x).__name__ == "SirPosterior" and (x.sims, x.now, x.horizons, x.squeezed) == (50, 4, (0, 2), False)
    assert tuple(x.counts.shape) == (2, 2, 2, 3) and tuple(x.accepted.shape) == (2, 2) and x.accepted_total().tolist() == [5, 0]
    assert x.counts.data_ptr() == r.counts.data_ptr() and x.accepted.data_ptr() == r.accepted.data_ptr()       # views
    assert torch.equal(x.counts, r.counts[:, 0]) and torch.equal(x.accepted, r.accepted[..., 0])


def test_one_evidence_object_drops_the_set_axis():
    import torch
    r, one = _result(), _result(squeezed=True)
    assert tuple(one.by_stratum().shape) == (3,) and one.by_stratum().tolist() == [5, 20, 75]
    assert tuple(one.marginals(error=0.1).shape) == (2, 3, 3) and torch.equal(one.marginals(error=0.1), r.marginals(error=0.1)[0])
    assert tuple(one.source(weights=[1, 1, 0]).shape) == (2,) and torch.equal(one.source(weights=[1, 1, 0]), r.source(weights=[1, 1, 0])[0])
    assert one.ess(error=0.1).ndim == 0 and float(one.ess(error=0.1)) == float(r.ess(error=0.1)[0])
    assert one.complete().ndim == 0 and bool(one.complete()) is True
    assert tuple(one.weights(0.2).shape) == (3,)                    # the weights know no set
    x = one.exact()
    assert x.squeezed and tuple(x.marginals().shape) == (2, 3, 3) and int(x.accepted_total()) == 5
