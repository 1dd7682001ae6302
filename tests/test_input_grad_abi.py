"""CPU: the built library exports the input-gradient entry points (include/gnode.h, ABI 223).  No compute call is made."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


def test_input_grad_entry_points_are_exported(lib):
    from gnode import _lib
    for name in ("gnode_backward_dx_f32", "gnode_backward_rk4_dx_f32"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert lib.gnode_version() >= 223


def test_null_outputs_are_refused(lib):
    """grads and gx both NULL is GNODE_ERR_ARG before any pointer is touched (null graph: the first check fails either way,
    so this only shows the call returns an error instead of crashing)"""
    st = lib.gnode_backward_dx_f32(None, None, None, None, 0, None, 0, None, None, 0, None, None, None, None, 1, 64, None, 0,
                                   None, 0, -1, None)
    assert st < 0
    st = lib.gnode_backward_rk4_dx_f32(None, None, None, None, 0, None, 0, None, None, None, None, None, 1, 64, None, 0, None,
                                       None)
    assert st < 0
    assert b"null" in lib.gnode_last_error()
