"""CPU: the scheduled DMP backward entries (include/gnode.h) are exported and bound with the header's arity, the version does not
move, the size query answers 0 for bad arguments, the entry refuses a call without a handle, and `dmp_marginals_schedule`
refuses what it must before the library is loaded or a DeviceGraph is made (no GPU here: both are made to raise)."""
import numpy as np
import pytest
import scipy.sparse as sp

ARG = -1                            # GNODE_ERR_ARG of include/gnode.h


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


ARITY = {"gnode_dmp_batch_schedule_backward_workspace_bytes": 3, "gnode_dmp_batch_schedule_backward_f32": 18}


def test_scheduled_backward_entries_exported(lib):
    from gnode import _lib
    for name, arity in ARITY.items():
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
        assert len(getattr(lib, name).argtypes) == arity, name
    assert len(lib.gnode_dmp_batch_schedule_f32.argtypes) == 14 and len(lib.gnode_dmp_batch_backward_f32.argtypes) == 16      # untouched
    assert lib.gnode_version() == 226                               # a stale library is known by the missing symbol


def test_the_unit_is_in_the_build_list():
    from gnode.build import SOURCES
    assert "gnode_dmp_schedule_bwd.hip" in SOURCES and "gnode_dmp_schedule.hip" in SOURCES and "gnode_dmp.hip" in SOURCES


def test_size_query_answers_zero_for_bad_arguments(lib):
    for B, T in ((4, 8), (0, 8), (4, 1), (-1, -1)):
        assert lib.gnode_dmp_batch_schedule_backward_workspace_bytes(None, B, T) == 0


def test_the_entry_refuses_a_call_without_a_handle(lib):
    """GNODE_ERR_ARG before anything is read: the other pointers are host arrays here and are never followed."""
    from gnode import _lib
    phase = np.zeros(4, dtype=np.int32)
    buf = np.zeros(64, dtype=np.float32)
    p = _lib.host_ptr(buf)
    rc = lib.gnode_dmp_batch_schedule_backward_f32(None, p, 0, p, 0, _lib.host_ptr(phase), 1, p, 1, 4, p, p, p, p, p, p, 1 << 20, None)
    assert rc == ARG and "null pointer" in lib.gnode_last_error().decode()
    assert not buf.any()


N, NNZ, B, T, P = 10, 18, 3, 5, 2
RP = np.concatenate([[0], np.cumsum([1] + [2] * 8 + [1])])
CI = np.asarray([j for i in range(N) for j in (i - 1, i + 1) if 0 <= j < N])
A = sp.csr_matrix((np.linspace(0.1, 0.5, NNZ), CI, RP), shape=(N, N))
PHASE = [0, 0, 1, 1, 0]


class Reached(Exception):
    pass


@pytest.fixture
def no_library(monkeypatch):
    from gnode import _lib, dmp

    def refuse(*a, **k):
        raise Reached("the library was loaded, or a DeviceGraph made")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(dmp, "DeviceGraph", refuse)


def _good():
    import torch
    return dict(weights=torch.full((P, NNZ), 0.3), gamma=torch.full((P, N), 0.2), init=torch.tensor([[0.8, 0.2, 0.0]]).repeat(B, N, 1),
                phase=PHASE)


def test_dmp_marginals_schedule_refuses_before_the_library(no_library):
    import torch
    from gnode.dmp import DmpGraph, dmp_marginals_schedule
    from gnode.ode_nn import rate_schedule
    G, ok = DmpGraph(A), _good()
    bad = [
        dict(graph=A), dict(graph=None),                                                    # not a DmpGraph
        dict(maxTime=1), dict(maxTime=0), dict(maxTime="soon"),
        dict(init=torch.zeros(0, N, 3)),                                                    # B < 1
        dict(init=torch.zeros(N, 3)), dict(init=torch.zeros(B, N - 1, 3)), dict(init=torch.zeros(B, N, 2)),
        dict(weights=torch.zeros(NNZ)), dict(weights=torch.zeros(P, NNZ + 1)), dict(weights=torch.zeros(B + 1, P, NNZ)),
        dict(weights=torch.zeros(B, P, NNZ, 1)),
        dict(gamma=torch.zeros(N)), dict(gamma=torch.zeros(P, N - 1)), dict(gamma=torch.zeros(B - 1, P, N)), dict(gamma=torch.zeros(0, N)),
        dict(weights=torch.zeros(P + 1, NNZ)), dict(gamma=torch.zeros(P + 1, N)),           # P disagrees between weights and gamma
        dict(weights=torch.zeros(B, P + 1, NNZ)), dict(gamma=torch.zeros(B, P - 1, N)),
        dict(weights=ok["weights"].double()), dict(gamma=ok["gamma"].double()), dict(init=ok["init"].double()),
        dict(weights=ok["weights"].numpy()), dict(gamma=0.2), dict(init=ok["init"].tolist()),
        dict(phase=[0, 0, 1, 2, 0]), dict(phase=[0, -1, 1, 1, 0]), dict(phase=[0, 0, 1, 1, P]),          # an entry outside [0, P)
        dict(phase=[0, 0, 1, 1]), dict(phase=[]),                                           # shorter than maxTime
        dict(phase=[0, 0.5, 1, 1, 0]), dict(phase=[[0, 0, 1, 1, 0]]), dict(phase="00110"), dict(phase=None),
        dict(phase=rate_schedule([0.1, 0.2, 0.3], starts=[1, 2, 3])),                       # a schedule of three phases, P = 2 tables
        dict(phase=rate_schedule([0.1, 0.2], steps=[0, 0, 1, 1])),                          # fewer steps than maxTime
        dict(weights=rate_schedule([ok["weights"]], starts=[1])), dict(gamma=rate_schedule([ok["gamma"]], starts=[1])),
    ]
    for change in bad:
        a = dict(graph=G, maxTime=T, **ok)
        a.update(change)
        with pytest.raises(ValueError):
            dmp_marginals_schedule(a["graph"], a["weights"], a["gamma"], a["init"], a["maxTime"], a["phase"])


def test_what_is_well_formed_reaches_the_device_check(no_library):
    """Well-formed tensors that are not on a GPU: GnodeError, as in dmp_marginals -- there is no CPU path.  Entry 0 of the phases
    is ignored, a longer phase list is cut, and a RateSchedule gives its phase_of_step."""
    from gnode import _lib
    from gnode.dmp import DmpGraph, dmp_marginals_schedule
    from gnode.ode_nn import rate_schedule
    ok = _good()
    for w, g in ((ok["weights"], ok["gamma"]), (ok["weights"].repeat(B, 1, 1), ok["gamma"].repeat(B, 1, 1))):
        for phase in (PHASE, [99, 0, 1, 1, 0], PHASE + [7, 7], np.asarray(PHASE, dtype=np.float64), rate_schedule(["a", "b"], starts=[1, 3]),
                      rate_schedule([None, None], steps=PHASE)):
            with pytest.raises(_lib.GnodeError):
                dmp_marginals_schedule(DmpGraph(A), w, g, ok["init"], T, phase)
        with pytest.raises(_lib.GnodeError):
            dmp_marginals_schedule(DmpGraph(A), w.clone().requires_grad_(), g, ok["init"], T, PHASE)


def test_dmp_marginals_still_refuses_a_schedule(no_library):
    import torch
    from gnode.dmp import DmpGraph, dmp_marginals
    from gnode.ode_nn import rate_schedule
    with pytest.raises(ValueError, match="RateSchedule"):
        dmp_marginals(DmpGraph(A), rate_schedule([torch.zeros(NNZ)], starts=[1]), torch.zeros(N), torch.zeros(1, N, 3), T)
