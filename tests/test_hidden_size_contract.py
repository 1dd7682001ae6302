"""CPU: every GN-ODE entry takes 4 <= H <= 128, H % 4 == 0 (include/gnode.h).  The forward, the RHS and the Euler backward
refuse any other H with GNODE_ERR_ARG in their argument checks, before anything is read from the graph but its size and
before anything is launched, and the forward and RHS workspace sizes are 0 there (no GPU needed;
tests/test_gpu_hidden_sizes.py repeats the forward and RHS checks on a real handle)."""
import ctypes as C

import pytest

ERR_ARG = -1
BAD_H = (0, 2, 6, 132, 256)


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


@pytest.fixture
def fake_graph():
    """A host stand-in for a graph handle of n = 34 nodes without hub rows (gnode_graph_s starts with int32 n; every
    other field zero).  The calls below fail their argument checks before any field but n and n_hub is read and before
    anything is launched."""
    buf = (C.c_int64 * 512)()
    C.cast(buf, C.POINTER(C.c_int32))[0] = 34
    return buf


def _params():
    from gnode import _lib
    p = _lib.Params()
    for f, _ in _lib.Params._fields_:
        setattr(p, f, 16)
    return p


def _forward(lib, g, H, n_steps=0, rows=34):
    vp = C.c_void_p
    dts = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)
    info = C.c_int32(0)
    return lib.gnode_forward_f32(g, vp(16), C.byref(_params()), C.cast(dts, vp), n_steps, 0, None, 0, vp(16), vp(16), vp(16),
                                 None, None, 0, rows, H, vp(16), 1 << 40, None, 0, C.byref(info))


def _rhs(lib, g, H, rows=34):
    vp = C.c_void_p
    return lib.gnode_rhs_f32(g, vp(16), vp(16), vp(16), vp(16), rows, H, vp(16), 1 << 40, None)


def _backward(lib, g, H, n_steps=2, rows=34):
    vp = C.c_void_p
    dts = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)
    return lib.gnode_backward_f32(g, vp(16), C.byref(_params()), C.cast(dts, vp), n_steps, None, 0, vp(16), None, 0,
                                  vp(16), vp(16), vp(16), C.byref(_params()), rows, H, vp(16), 1 << 40, None, 0, -1)


@pytest.mark.parametrize("H", BAD_H)
@pytest.mark.parametrize("entry", ["forward", "forward_steps", "rhs", "backward"])
def test_entries_refuse_unsupported_hidden_sizes(entry, H, lib, fake_graph):
    g = C.cast(fake_graph, C.c_void_p)
    call = {"forward": lambda: _forward(lib, g, H), "forward_steps": lambda: _forward(lib, g, H, n_steps=3),
            "rhs": lambda: _rhs(lib, g, H), "backward": lambda: _backward(lib, g, H)}[entry]
    assert call() == ERR_ARG
    assert "H" in lib.gnode_last_error().decode()


@pytest.mark.parametrize("H", BAD_H)
def test_workspace_sizes_are_zero_outside_the_range(H, lib, fake_graph):
    g = C.cast(fake_graph, C.c_void_p)
    assert lib.gnode_forward_workspace_bytes(g, 34, H, 0) == 0
    assert lib.gnode_forward_workspace_bytes(g, 34, H, 1) == 0
    assert lib.gnode_rhs_workspace_bytes(g, 34, H) == 0
    assert lib.gnode_rhs_vjp_workspace_bytes(g, 34, H) == 0


@pytest.mark.parametrize("H", [4, 68, 124, 128])
def test_workspace_sizes_inside_the_range(H, lib, fake_graph):
    g = C.cast(fake_graph, C.c_void_p)
    assert lib.gnode_forward_workspace_bytes(g, 34, H, 0) > 0
    assert lib.gnode_rhs_workspace_bytes(g, 34, H) > 0
    assert lib.gnode_backward_workspace_bytes(g, 34, H) > 0
