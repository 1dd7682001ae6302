"""What the host tests of the Monte-Carlo candidate sweep share (tests/test_sir_{sweep,score,timed,post,strata}_host.py and
tests/test_sir_mc_launches.py): the 6-ring, the library out of reach, the built library, a hand-made evidence object and the
refusals every scorer inherits from the checks it shares with `outbreak_sizes_mc`."""
from types import SimpleNamespace

import numpy as np
import pytest


class Reached(Exception):
    pass


@pytest.fixture
def no_library(monkeypatch):
    from gnode import _lib, ode_nn

    def refuse(*a, **k):
        raise Reached("the library was loaded, or a DeviceGraph made")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(ode_nn, "DeviceGraph", refuse)


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


N = 6
RING = (np.arange(0, 2 * N + 1, 2), np.asarray([j % N for i in range(N) for j in sorted(((i - 1) % N, (i + 1) % N))]))


def _obs(rows, offsets, n=N):
    return SimpleNamespace(rows=np.asarray(rows), row_offsets=np.asarray(offsets), n=n)


def shared_refusals():
    """What outbreak_sizes_mc refuses, through the shared checks: changes to a call that is in order on RING with candidates
    [0, 3, -1] and maxTime 4."""
    from gnode.ode_nn import InitialState, edge_rates, rate_schedule
    short = rate_schedule([0.2, 0.4], steps=[0, 0, 0, 1, 1, 0])     # names 6 entries: calendar steps up to 5
    return [
        dict(shifts=[0, -1, 2]), dict(shifts=[0, 1]), dict(shifts="now"), dict(gamma=short, shifts=[0, 3, 0]), dict(gamma=short, maxTime=7),
        dict(beta=1.5), dict(beta=float("nan")), dict(gamma=-0.1), dict(beta=[0.3] * (N - 1)), dict(gamma=edge_rates(RING, np.full(2 * N, 0.3))),
        dict(candidates=[0, N]), dict(candidates=[-2]), dict(candidates=[]), dict(candidates=[0.5]),
        dict(start=[N]), dict(start=InitialState.from_sets(N + 1, [1])),
        dict(maxTime=0), dict(maxTime=2.5), dict(sims=-1), dict(sims=2.5), dict(sim_offset=-1), dict(sims=10, sim_offset=2**32),
    ]
