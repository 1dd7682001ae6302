"""CPU: the float64 restatements of the RHS vector-Jacobian product and of the RK4 adjoint (oracle/gnode_restate.py)
against what the REFERENCE's classes produced through torch autograd (tests/golden/make_golden_rhs_vjp.py,
make_golden_rk4_adjoint.py), and the argument checks of the two new C entries (no GPU: every call is refused before
anything is launched)."""
import ctypes as C

import numpy as np
import pytest

import gnode_restate as RS
from fixture_cases import VJP_CASES, load_multi_case, load_vjp_case, rk4_case


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30)


@pytest.mark.parametrize("name", VJP_CASES)
def test_vjp_restatement_vs_reference(name):
    rp, ci, y, v, P, d = load_vjp_case(name)
    if name == "rhs_vjp_heavy_B1_H64":
        assert int(np.diff(rp).max()) > 96                      # hub rows (GN_HUB_T) in the graph
    _, gy, gW, gb = RS.rhs_vjp_np(y, P["odefunc.linear.weight"], P["odefunc.linear.bias"], v, rp, ci)
    assert _rel(gy[d["rows_kept"]], d["gx"]) <= 1e-9
    assert _rel(gW, d["gW"]) <= 1e-9
    assert _rel(gb, d["gb"]) <= 1e-9


def test_vjp_restatement_vs_reference_multi():
    import gnode_oracle as O
    graphs, picks, y, v, P, d = load_multi_case()
    rp, ci, off = O.concat_csr(graphs, picks)
    tot, H = y.shape[1], y.shape[2]
    _, gy, gW, gb = RS.rhs_vjp_np(y.reshape(4 * tot, H), P["odefunc.linear.weight"], P["odefunc.linear.bias"],
                                 v.reshape(4 * tot, H), rp, ci)
    assert _rel(gy.reshape(4, tot, H), d["gx"]) <= 1e-9
    assert _rel(gW, d["gW"]) <= 1e-9 and _rel(gb, d["gb"]) <= 1e-9


def _rk4_fixture_adjoint(name, method):
    """(the restated adjoint of `method` on an RK4-adjoint fixture's inputs for the reference's L1 loss, fixture dict)"""
    import gnode_oracle as O
    from gnode import ops
    rp, ci, x, P, y, d = rk4_case(name)
    maxTime, deltaT = int(d["maxTime"]), float(d["deltaT"])
    return RS.adjoint(x.reshape(-1, x.shape[-1]), P, (rp, ci), O.step_sizes(O.time_grid(maxTime, deltaT)),
                     RS.l1_loss_of(y, ops.subsample_rows(maxTime, deltaT)), method), d


@pytest.mark.parametrize("name", ["rk4_adjoint_karate_H64_T20", "rk4_adjoint_loops40_H8_T5"])
def test_rk4_adjoint_restatement_vs_reference(name):
    got, d = _rk4_fixture_adjoint(name, "rk4")
    for k in RS.KEYS:
        g = got[k]
        if k == "linearS2.bias":                                 # exact gradient 0 (softmax shift invariance)
            assert abs(float(g[0])) <= 1e-12 and abs(float(d["G:" + k][0])) <= 1e-12
            continue
        assert _rel(g, d["G:" + k]) <= 1e-9, k


def test_rk4_and_euler_adjoints_differ():
    """The RK4 fixtures are not the Euler rule in disguise: the Euler restatement on the same inputs is far off."""
    eu, d = _rk4_fixture_adjoint("rk4_adjoint_karate_H64_T20", "euler")
    assert _rel(eu["odefunc.linear.weight"], d["G:odefunc.linear.weight"]) > 1e-3


# --------------------------------------------------------------------------- argument checks of the C entries
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
    anything is launched; a real handle needs a GPU (tests/test_gpu_rhs_vjp.py repeats these checks on one)."""
    buf = (C.c_int64 * 512)()
    C.cast(buf, C.POINTER(C.c_int32))[0] = 34
    return buf


def _vjp(lib, g, y=1, H=8, rows=34, ws=1, wsb=1 << 40):
    vp = C.c_void_p
    return lib.gnode_rhs_vjp_f32(g, vp(y) if y else None, vp(16), vp(16), vp(16), None, vp(16), None, None, rows, H,
                                 vp(ws) if ws else None, wsb, None)


def test_rhs_vjp_argument_checks(lib, fake_graph):
    from gnode import _lib
    g = C.cast(fake_graph, C.c_void_p)
    ERR_ARG, ERR_WS = -1, -3
    assert _vjp(lib, None) == ERR_ARG                          # null graph
    assert _vjp(lib, g, y=0) == ERR_ARG                        # null state
    assert _vjp(lib, g, ws=0) == ERR_ARG                       # null workspace
    for H in (0, 2, 6, 132, 256):
        assert _vjp(lib, g, H=H) == ERR_ARG, H                 # 4 <= H <= 128, H % 4 == 0
    assert _vjp(lib, g, rows=35) == ERR_ARG                    # rows not a multiple of n
    assert _vjp(lib, g, rows=0) == ERR_ARG
    need = lib.gnode_rhs_vjp_workspace_bytes(g, 68, 8)
    assert need > 0
    assert _vjp(lib, g, rows=68, wsb=need - 1) == ERR_WS       # short workspace
    assert "workspace" in _lib.load().gnode_last_error().decode()
    assert lib.gnode_rhs_vjp_workspace_bytes(None, 68, 8) == 0
    assert lib.gnode_rhs_vjp_workspace_bytes(g, 68, 6) == 0


def _rk4(lib, g, H=8, rows=34, n_steps=3, ws=1, wsb=1 << 40, p_ok=True, grads_ok=True, sol=1):
    from gnode import _lib
    vp = C.c_void_p
    p, gp = _lib.Params(), _lib.Params()
    for f, _ in _lib.Params._fields_:
        setattr(p, f, 16 if p_ok else None)
        setattr(gp, f, 16 if grads_ok else None)
    dts = (C.c_float * 8)(*([0.5] * 8))
    return lib.gnode_backward_rk4_f32(g, vp(16), C.byref(p), C.cast(dts, vp), n_steps, None, 0, vp(sol) if sol else None,
                                      vp(16), vp(16), vp(16), C.byref(gp), rows, H, vp(ws) if ws else None, wsb, None)


def test_backward_rk4_argument_checks(lib, fake_graph):
    g = C.cast(fake_graph, C.c_void_p)
    ERR_ARG, ERR_WS = -1, -3
    assert _rk4(lib, None) == ERR_ARG
    assert _rk4(lib, g, sol=0) == ERR_ARG
    assert _rk4(lib, g, ws=0) == ERR_ARG
    assert _rk4(lib, g, p_ok=False) == ERR_ARG
    assert _rk4(lib, g, grads_ok=False) == ERR_ARG
    assert _rk4(lib, g, n_steps=-1) == ERR_ARG
    for H in (0, 6, 132):
        assert _rk4(lib, g, H=H) == ERR_ARG, H
    assert _rk4(lib, g, rows=50) == ERR_ARG
    need = lib.gnode_backward_rk4_workspace_bytes(g, 34, 8)
    assert need > 0
    assert _rk4(lib, g, wsb=need - 1) == ERR_WS
