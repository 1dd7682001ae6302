"""CPU: the per-trajectory Monte-Carlo entry (gnode_sir_mc_philox_traj, include/gnode.h) is exported and bound without a
version step, and `sir_trajectories` refuses bad arguments before the library is entered (no GPU here: a stub graph is
all these calls may touch)."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


def test_traj_entries_exported(lib):
    from gnode import _lib
    for name in ("gnode_sir_traj_workspace_bytes", "gnode_sir_mc_philox_traj"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert len(lib.gnode_sir_mc_philox_traj.argtypes) == 18
    assert lib.gnode_sir_traj_workspace_bytes(None, 20) == 0           # no handle: no guess
    assert lib.gnode_version() == 226                                  # a stale library is known by the missing symbol


def test_missing_symbol_is_reported_as_stale(lib, monkeypatch):
    """An ABI entry that the loaded library lacks raises the "is stale ... rebuild it" error, not an AttributeError."""
    from gnode import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.ABI, "gnode_entry_of_a_later_build", (_lib._int, []))
    with pytest.raises(_lib.GnodeError, match=r"is stale .*gnode_entry_of_a_later_build.*rebuild it"):
        _lib.load()


class _StubGraph:
    """What sir_trajectories reads before it enters the library.  `handle` raises: reaching it means the check came too late."""
    n = 10

    @property
    def handle(self):
        raise AssertionError("the library was entered before the arguments were checked")


def _bad_rates():
    ok = np.full(10, 0.3)
    yield "wrong length", np.full(9, 0.3)
    yield "two-dimensional", np.full((10, 1), 0.3)
    for what, x in (("negative", -0.1), ("above one", 1.5), ("NaN", float("nan"))):
        a = ok.copy()
        a[6] = x
        yield what, a


@pytest.mark.parametrize("what,bad", list(_bad_rates()), ids=[w for w, _ in _bad_rates()])
def test_sir_trajectories_refuses_bad_rates(what, bad):
    from gnode.ode_nn import sir_trajectories
    for kw in ({"beta": bad, "gamma": 0.2}, {"beta": 0.3, "gamma": bad.tolist()}, {"beta": np.full(10, 0.3), "gamma": bad}):
        with pytest.raises(ValueError):
            sir_trajectories(_StubGraph(), [0], sims=4, T=3, rng_seed=1, device="cpu", **kw)
    with pytest.raises(ValueError):                                    # the scalar side of a mixed call
        sir_trajectories(_StubGraph(), [0], np.full(10, 0.3), 1.5, sims=4, T=3, rng_seed=1, device="cpu")


def test_sir_trajectories_refuses_long_T_and_no_output():
    from gnode.ode_nn import sir_trajectories
    with pytest.raises(ValueError, match="32767"):
        sir_trajectories(_StubGraph(), [0], 0.3, 0.2, sims=4, T=40000, rng_seed=1, device="cpu")
    with pytest.raises(ValueError, match="neither"):
        sir_trajectories(_StubGraph(), [0], 0.3, 0.2, sims=4, T=3, rng_seed=1, events=False, curves=False, device="cpu")


def test_event_helpers_state_the_invariants():
    """The three torch helpers on a hand-written pair of trajectories (CPU tensors: they run on the tensors' device)."""
    import torch
    from gnode.ode_nn import sir_counts_from_events, sir_curves_from_events, sir_state_at
    t_inf = torch.tensor([[0, 1, 2, -1], [0, -1, 1, -1]], dtype=torch.int16)
    t_rec = torch.tensor([[1, 3, -1, -1], [-1, -1, 2, -1]], dtype=torch.int16)
    assert sir_state_at(t_inf, t_rec, 0).tolist() == [[1, 0, 0, 0], [1, 0, 0, 0]]
    assert sir_state_at(t_inf, t_rec, 2).tolist() == [[2, 1, 1, 0], [1, 0, 2, 0]]
    assert sir_state_at(t_inf, t_rec, 2).dtype == torch.int8
    cv = sir_curves_from_events(t_inf, t_rec, 4)
    assert cv.dtype == torch.int32 and cv.tolist() == [[[3, 1, 0], [2, 1, 1], [1, 2, 1], [1, 1, 2]],
                                                        [[3, 1, 0], [2, 2, 0], [2, 1, 1], [2, 1, 1]]]
    cn = sir_counts_from_events(t_inf, t_rec, 4)
    assert cn.dtype == torch.int32 and cn.shape == (3, 4, 4)
    assert cn[:, 0].tolist() == [[0, 1, 1, 1], [1, 0, 0, 0], [0, 0, 0, 0]]       # row 0: the initial state once
    assert cn[:, 2].tolist() == [[0, 1, 0, 2], [1, 1, 1, 0], [1, 0, 1, 0]]
