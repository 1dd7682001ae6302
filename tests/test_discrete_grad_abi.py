"""CPU: the built library exports the exact Euler gradient's entry points (include/gnode.h, ABI 224).  No compute call is
made."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


def test_discrete_entry_points_are_exported(lib):
    from gnode import _lib
    for name in ("gnode_backward_discrete_workspace_bytes", "gnode_backward_discrete_f32"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert lib.gnode_version() >= 224


def test_bad_calls_are_refused(lib):
    """NULL grads and NULL gx, and a trajectory a keep buffer was filled with (GNODE_SOL_KEEP = 2), are GNODE_ERR_ARG before
    any pointer is touched; so is a null graph"""
    st = lib.gnode_backward_discrete_f32(None, None, None, None, 0, None, 0, None, -1, None, None, None, None, None, 1, 64,
                                         None, 0, None)
    assert st == -1 and b"neither" in lib.gnode_last_error()
    st = lib.gnode_backward_discrete_f32(None, None, None, None, 0, None, 0, None, 2, None, None, None, None, 16, 1, 64,
                                         None, 0, None)
    assert st == -1 and b"keep" in lib.gnode_last_error()
    st = lib.gnode_backward_discrete_f32(None, None, None, None, 0, None, 0, None, 1, None, None, None, None, 16, 1, 64,
                                         None, 0, None)
    assert st == -1 and b"null" in lib.gnode_last_error()
    assert lib.gnode_backward_discrete_workspace_bytes(None, 1, 64) == 0


def test_rk4_is_refused_without_a_gpu():
    """ODEBlock(adjoint=False) is Euler only: the constructor says so before anything runs"""
    from gnode import _lib
    from gnode.ode_nn_ngraph_sim import _check_adjoint
    assert _check_adjoint(True, "rk4") is True and _check_adjoint(False, "euler") is False
    with pytest.raises(_lib.GnodeError, match="Euler only"):
        _check_adjoint(False, "rk4")


@pytest.mark.parametrize("value, want", [("0", False), ("1", True), (None, True)])
def test_trainer_knob_is_read_at_import(value, want):
    """GNODE_ADJOINT=0 switches the drop-in scripts to the exact gradient; unset or 1 keeps the adjoint (a fresh interpreter:
    the knob is read once, at import)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "GNODE_ADJOINT"}
    if value is not None:
        env["GNODE_ADJOINT"] = value
    r = subprocess.run([sys.executable, "-c", "from gnode import trainer; print(trainer.ADJOINT_DEFAULT)"], cwd=root,
                       env=dict(env, PYTHONPATH=os.path.join(root, "gn-ode-sir_amd")), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == str(want)
