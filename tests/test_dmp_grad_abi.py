"""CPU: the DMP backward entries (include/gnode.h) are exported and bound with the header's arity, the version does not move,
the size queries answer 0 without a handle, and `dmp_marginals` refuses what it must before the library is loaded or a
DeviceGraph is made (no GPU here: both are made to raise)."""
import numpy as np
import pytest
import scipy.sparse as sp


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


ARITY = {"gnode_dmp_batch_backward_lds_bytes": 1, "gnode_dmp_batch_backward_workspace_bytes": 3, "gnode_dmp_batch_backward_f32": 16,
         "gnode_dmp_backward_workspace_bytes": 2, "gnode_dmp_backward_f32": 13}


def test_backward_entries_exported(lib):
    from gnode import _lib
    for name, arity in ARITY.items():
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
        assert len(getattr(lib, name).argtypes) == arity, name
    assert len(lib.gnode_dmp_batch_f32.argtypes) == 12 and len(lib.gnode_dmp_init_f32.argtypes) == 9      # untouched
    assert lib.gnode_version() == 226                               # a stale library is known by the missing symbol


def test_size_queries_answer_zero_without_a_handle(lib):
    assert lib.gnode_dmp_batch_backward_lds_bytes(None) == 0
    assert lib.gnode_dmp_batch_backward_workspace_bytes(None, 4, 8) == 0
    assert lib.gnode_dmp_backward_workspace_bytes(None, 8) == 0


N, NNZ, B, T = 10, 18, 3, 5
RP = np.concatenate([[0], np.cumsum([1] + [2] * 8 + [1])])
CI = np.asarray([j for i in range(N) for j in (i - 1, i + 1) if 0 <= j < N])
A = sp.csr_matrix((np.linspace(0.1, 0.5, NNZ), CI, RP), shape=(N, N))


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
    return dict(weights=torch.full((NNZ,), 0.3), gamma=torch.full((N,), 0.2), init=torch.tensor([[0.8, 0.2, 0.0]]).repeat(B, N, 1))


def test_dmp_marginals_refuses_before_the_library(no_library):
    import torch
    from gnode.dmp import DmpGraph, dmp_marginals
    G, ok = DmpGraph(A), _good()
    bad = [
        dict(graph=A), dict(graph=None),                                                    # not a DmpGraph
        dict(maxTime=1), dict(maxTime=0),
        dict(init=torch.zeros(0, N, 3)),                                                    # B < 1
        dict(init=torch.zeros(N, 3)), dict(init=torch.zeros(B, N - 1, 3)), dict(init=torch.zeros(B, N, 2)),
        dict(weights=torch.zeros(NNZ + 1)), dict(weights=torch.zeros(B + 1, NNZ)), dict(weights=torch.zeros(B, NNZ, 1)),
        dict(gamma=torch.zeros(N - 1)), dict(gamma=torch.zeros(B - 1, N)), dict(gamma=torch.zeros(())),
        dict(weights=ok["weights"].double()), dict(gamma=ok["gamma"].double()), dict(init=ok["init"].double()),
        dict(weights=ok["weights"].numpy()), dict(gamma=0.2), dict(init=ok["init"].tolist()),
    ]
    for change in bad:
        a = dict(graph=G, maxTime=T, **ok)
        a.update(change)
        with pytest.raises(ValueError):
            dmp_marginals(a["graph"], a["weights"], a["gamma"], a["init"], a["maxTime"])


def test_dmp_marginals_refuses_cpu_tensors(no_library):
    """Well-formed tensors that are not on a GPU: GnodeError, as everywhere else -- there is no CPU path."""
    from gnode import _lib
    from gnode.dmp import DmpGraph, dmp_marginals
    ok = _good()
    for w, g in ((ok["weights"], ok["gamma"]), (ok["weights"].repeat(B, 1), ok["gamma"].repeat(B, 1))):
        with pytest.raises(_lib.GnodeError):
            dmp_marginals(DmpGraph(A), w, g, ok["init"], T)
        with pytest.raises(_lib.GnodeError):
            dmp_marginals(DmpGraph(A), w.requires_grad_(), g, ok["init"], T)
