"""CPU: the differentiable mean-field's entries (include/gnode.h) are exported and bound with the header's arity, the version
does not move, the size query answers 0 without a handle, the entries refuse a null handle, and `meanfield_marginals` refuses
what it must before the library is loaded (no GPU here: a stub graph is all it may touch)."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


ARITY = {"gnode_meanfield_rates_steps_f64": 21, "gnode_meanfield_rates_backward_workspace_bytes": 3, "gnode_meanfield_rates_backward_f64": 24}
ARG = -1                            # GNODE_ERR_ARG of include/gnode.h


def test_entries_exported(lib):
    from gnode import _lib
    for name, arity in ARITY.items():
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
        assert len(getattr(lib, name).argtypes) == arity, name
    assert len(lib.gnode_meanfield_rates_f64.argtypes) == 17        # untouched
    assert lib.gnode_version() == 226                               # a stale library is known by the missing symbol


def test_size_query_answers_zero_without_a_handle(lib):
    assert lib.gnode_meanfield_rates_backward_workspace_bytes(None, 4, 8) == 0


def test_entries_refuse_a_null_handle(lib):
    """in front of any HIP call: this runs without a GPU"""
    t_out, h, n_acc = np.array([0.0, 1.0]), np.array([1.0]), np.array([0, 1], np.int32)
    steps, n_h = C.c_int64(-7), C.c_int64(-7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = lib.gnode_meanfield_rates_steps_f64(None, 1, None, None, None, None, p(t_out), 2, 1e-8, 1e-10, None, None, None, C.byref(steps),
                                             None, 0, None, p(h), 1, C.byref(n_h), p(n_acc))
    assert rc == ARG and b"null pointer" in lib.gnode_last_error()
    assert steps.value == -7 and n_h.value == -7 and list(n_acc) == [0, 1] and h[0] == 1.0
    rc = lib.gnode_meanfield_rates_backward_f64(None, 1, None, None, None, None, p(t_out), 2, p(h), 1, p(n_acc), *([None] * 10), None, 0, None)
    assert rc == ARG and b"gnode_meanfield_rates_backward_f64: null pointer" in lib.gnode_last_error()


N, NNZ, B, T = 10, 18, 3, 5


class _StubGraph:
    """What meanfield_marginals reads before it enters the library.  `handle` raises: reaching it means a check came too late."""
    n, nnz = N, NNZ

    @property
    def handle(self):
        raise AssertionError("the library was entered before the arguments were checked")


@pytest.fixture
def no_library(monkeypatch):
    from gnode import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", refuse)


def _good():
    import torch
    f = torch.float64
    return dict(init=torch.tensor([[0.8, 0.2, 0.0]], dtype=f).repeat(B, N, 1), beta=torch.full((B, N), 0.3, dtype=f),
                gamma=torch.full((N,), 0.2, dtype=f), w=torch.full((NNZ,), 0.5, dtype=f))


def test_meanfield_marginals_refuses_before_the_library(no_library):
    import torch
    from gnode.ode_nn import meanfield_marginals
    ok, f = _good(), torch.float64
    bad = [
        dict(init=torch.zeros(0, N, 3, dtype=f)),                                           # B < 1
        dict(init=torch.zeros(N, 3, dtype=f)), dict(init=torch.zeros(B, N - 1, 3, dtype=f)), dict(init=torch.zeros(B, N, 2, dtype=f)),
        dict(beta=torch.zeros(N + 1, dtype=f)), dict(beta=torch.zeros(B + 1, N, dtype=f)), dict(beta=torch.zeros((), dtype=f)),
        dict(gamma=torch.zeros(N - 1, dtype=f)), dict(gamma=torch.zeros(B - 1, N, dtype=f)), dict(gamma=torch.zeros(B, N, 1, dtype=f)),
        dict(w=torch.zeros(NNZ + 1, dtype=f)), dict(w=torch.zeros(B, NNZ, dtype=f)),
        dict(init=ok["init"].float()), dict(beta=ok["beta"].float()), dict(gamma=ok["gamma"].float()), dict(w=ok["w"].float()),
        dict(init=ok["init"].numpy()), dict(beta=0.3), dict(gamma=0.2), dict(gamma=None), dict(w=ok["w"].tolist()),
        dict(maxTime=0), dict(deltaT=0),
    ]
    for change in bad:
        a = dict(maxTime=T, deltaT=1, **ok)
        a.update(change)
        with pytest.raises(ValueError):
            meanfield_marginals(_StubGraph(), a["init"], a["beta"], a["gamma"], a["w"], deltaT=a["deltaT"], maxTime=a["maxTime"])


def test_meanfield_marginals_refuses_cpu_tensors(no_library):
    """Well-formed tensors that are not on a GPU: GnodeError, as everywhere else -- there is no CPU path."""
    from gnode import _lib
    from gnode.ode_nn import meanfield_marginals
    ok = _good()
    for beta, w in ((ok["beta"], ok["w"]), (None, None), (ok["beta"][0].clone().requires_grad_(), ok["w"])):
        with pytest.raises(_lib.GnodeError):
            meanfield_marginals(_StubGraph(), ok["init"], beta, ok["gamma"], w, maxTime=T)
