"""GPU: the RHS vector-Jacobian product (gnode_rhs_vjp_f32, ops.rhs_vjp) against the reference's classes (fixtures of
tests/golden/make_golden_rhs_vjp.py) and the float64 restatement, and the differentiable ODEfunc built on it."""
import ctypes as C

import numpy as np
import pytest

import fixture_cases as FC
import gnode_restate as RS
from fixture_cases import VJP_CASES, load_multi_case, load_vjp_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30)


def _run(dev, rp, ci, y, v, P, want_f=True):
    import torch
    from gnode import ops
    from gnode.graph import DeviceGraph
    g = DeviceGraph(rp, ci)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    W, b = t(P["odefunc.linear.weight"]), t(P["odefunc.linear.bias"])
    yt, vt = t(y), t(v)
    out = ops.rhs_vjp(g, yt, W, b, vt, want_f=want_f)
    return g, yt, W, b, vt, out


@pytest.mark.parametrize("name", VJP_CASES)
def test_rhs_vjp_vs_reference_classes(name, dev):
    import torch
    from gnode import ops
    rp, ci, y, v, P, d = load_vjp_case(name)
    g, yt, W, b, vt, (f, gy, gW, gb) = _run(dev, rp, ci, y, v, P)
    assert _rel(gy.cpu().numpy()[d["rows_kept"]], d["gx"]) <= 1e-5
    assert _rel(gW.cpu().numpy(), d["gW"]) <= 1e-4
    assert _rel(gb.cpu().numpy(), d["gb"]) <= 1e-4
    # f is gnode_rhs_f32's, bit for bit
    assert torch.equal(f, ops.rhs(g, yt, W, b))
    # deterministic: a second call gives the same bits
    f2, gy2, gW2, gb2 = ops.rhs_vjp(g, yt, W, b, vt, want_f=True)
    assert torch.equal(f, f2) and torch.equal(gy, gy2) and torch.equal(gW, gW2) and torch.equal(gb, gb2)
    # each output alone is the same as all together
    _, gy3, _, _ = ops.rhs_vjp(g, yt, W, b, vt, want_W=False, want_b=False)
    _, _, gW3, gb3 = ops.rhs_vjp(g, yt, W, b, vt, want_y=False)
    assert torch.equal(gy, gy3) and torch.equal(gW, gW3) and torch.equal(gb, gb3)


def test_rhs_vjp_vs_reference_classes_multi(dev):
    import gnode_oracle as O
    graphs, picks, y, v, P, d = load_multi_case()
    rp, ci, _ = O.concat_csr(graphs, picks)
    tot, H = y.shape[1], y.shape[2]
    _, _, _, _, _, (f, gy, gW, gb) = _run(dev, rp, ci, y.reshape(4 * tot, H), v.reshape(4 * tot, H), P)
    assert _rel(gy.cpu().numpy().reshape(4, tot, H), d["gx"]) <= 1e-5
    assert _rel(gW.cpu().numpy(), d["gW"]) <= 1e-4 and _rel(gb.cpu().numpy(), d["gb"]) <= 1e-4


@pytest.mark.parametrize("kind,n,m,B,H", [
    ("er", 300, 1200, 2, 4), ("er", 300, 1200, 3, 8), ("er", 257, 900, 2, 24), ("er", 500, 2500, 2, 64),
    ("er", 200, 800, 2, 128), ("cl", 2000, 12000, 2, 8), ("cl", 2000, 12000, 1, 64), ("cl", 1500, 9000, 1, 128),
    ("er", 75000, 300000, 4, 64),
])
def test_rhs_vjp_vs_restatement(kind, n, m, B, H, dev):
    import gnode_oracle as O
    from gnode import synth
    rp, ci = synth.er_csr(n, m, seed=n + H) if kind == "er" else O.chung_lu_graph(n, m, seed=n + H)[:2]
    y, v = FC.vjp_inputs(B * n, H, seed=H, sample_rows=n)
    P = synth.linear_params(H, seed=H + 7)
    _, _, _, _, _, (f, gy, gW, gb) = _run(dev, rp, ci, y, v, P)
    wf, wy, wW, wb = RS.rhs_vjp_np(y, P["odefunc.linear.weight"], P["odefunc.linear.bias"], v, rp, ci)
    assert _rel(f.cpu().numpy(), wf) <= 1e-5
    assert _rel(gy.cpu().numpy(), wy) <= 1e-5
    assert _rel(gW.cpu().numpy(), wW) <= 1e-4 and _rel(gb.cpu().numpy(), wb) <= 1e-4


def test_rhs_vjp_argument_checks_on_a_real_handle(dev):
    import torch
    from gnode import _lib
    from gnode.graph import DeviceGraph
    from gnode import synth
    lib = _lib.load()
    rp, ci = synth.er_csr(50, 150, seed=1)
    g = DeviceGraph(rp, ci)
    y = torch.zeros((4 * 100, 8), device=dev)
    need = lib.gnode_rhs_vjp_workspace_bytes(g.handle, 100, 8)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    call = lambda rows, H, wsb: lib.gnode_rhs_vjp_f32(g.handle, _lib.ptr(y), _lib.ptr(y), _lib.ptr(y), _lib.ptr(y), None,
                                                      _lib.ptr(y), None, None, rows, H, _lib.ptr(ws), wsb, _lib.stream_ptr())
    assert call(99, 8, need) == -1
    assert call(100, 6, need) == -1
    assert call(100, 8, need - 1) == -3
    assert call(100, 8, need) == 0
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- the differentiable ODEfunc
def _integrate(f, y0, dts, method):
    y = y0
    for dt in dts:
        if method == "euler":
            y = y + dt * f(0.0, y)
        else:
            y = y + RS.rk4_step(lambda s: f(0.0, s), y, dt)
    return y


@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("H", [8, 64])
def test_differentiable_odefunc_single(method, H, dev):
    """A plain Python integrator around ODEfunc(..., differentiable=True) trains: its gradients (state, W, b) match torch
    autograd through the float64 restatement of the same loop."""
    import torch
    import scipy.sparse as sp
    from gnode import synth
    from gnode.ode_nn_ngraph_sim import ODEfunc
    n, B = 120, 2
    rp, ci = synth.er_csr(n, 400, seed=5)
    A = sp.csr_matrix((np.ones(ci.shape[0]), ci, rp), shape=(n, n))
    f = ODEfunc(A, 0.2, 0.1, H, dev, differentiable=True).to(dev)
    P = synth.linear_params(H, seed=3)
    with torch.no_grad():
        f.linear.weight.copy_(torch.from_numpy(P["odefunc.linear.weight"]))
        f.linear.bias.copy_(torch.from_numpy(P["odefunc.linear.bias"]))
    y0, w = FC.vjp_inputs(B * n, H, seed=9, sample_rows=n)
    y0[:3 * B * n] *= 0.5
    dts = [0.5, 0.5, 0.25]
    yt = torch.from_numpy(y0).to(dev).requires_grad_(True)
    loss = (_integrate(f, yt, dts, method) * torch.from_numpy(w).to(dev)).sum()
    loss.backward()
    # float64 restatement through autograd
    ridx, cidx = RS.index(rp, ci, B * n)
    W64 = torch.from_numpy(P["odefunc.linear.weight"]).double().requires_grad_(True)
    b64 = torch.from_numpy(P["odefunc.linear.bias"]).double().requires_grad_(True)
    y64 = torch.from_numpy(y0).double().requires_grad_(True)
    f64 = lambda t, y: RS.rhs(y, W64, b64, ridx, cidx)
    L64 = (_integrate(f64, y64, dts, method) * torch.from_numpy(w).double()).sum()
    L64.backward()
    assert abs(float(loss) - float(L64)) <= 1e-4 * max(1.0, abs(float(L64)))
    assert _rel(yt.grad.cpu().numpy(), y64.grad.numpy()) <= 1e-4
    assert _rel(f.linear.weight.grad.cpu().numpy(), W64.grad.numpy()) <= 1e-4
    assert _rel(f.linear.bias.grad.cpu().numpy(), b64.grad.numpy()) <= 1e-4


@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_differentiable_odefunc_multi(method, dev):
    import torch
    import gnode_oracle as O
    from gnode.ode_nn_ngraphs import ODEfunc
    import scipy.sparse as sp
    graphs, picks, y, w, P, d = load_multi_case()
    H = y.shape[2]
    A_list = [sp.csr_matrix((np.ones(ci.shape[0]), ci, rp), shape=(rp.shape[0] - 1,) * 2) for rp, ci in graphs]
    f = ODEfunc(A_list, H, dev, differentiable=True).to(dev)
    with torch.no_grad():
        f.linear.weight.copy_(torch.from_numpy(P["odefunc.linear.weight"]))
        f.linear.bias.copy_(torch.from_numpy(P["odefunc.linear.bias"]))
    y[:3] *= 0.5
    dts = [0.5, 0.5]
    yt = torch.from_numpy(y).to(dev).requires_grad_(True)
    loss = (_integrate(f, yt, dts, method) * torch.from_numpy(w).to(dev)).sum()
    loss.backward()
    rp, ci, _ = O.concat_csr(graphs, picks)
    tot = y.shape[1]
    ridx, cidx = RS.index(rp, ci, tot)
    W64 = torch.from_numpy(P["odefunc.linear.weight"]).double().requires_grad_(True)
    b64 = torch.from_numpy(P["odefunc.linear.bias"]).double().requires_grad_(True)
    y64 = torch.from_numpy(y).double().requires_grad_(True)
    f64 = lambda t, s: RS.rhs(s.reshape(4 * tot, H), W64, b64, ridx, cidx).view_as(s)
    L64 = (_integrate(f64, y64, dts, method) * torch.from_numpy(w).double()).sum()
    L64.backward()
    assert _rel(yt.grad.cpu().numpy(), y64.grad.numpy()) <= 1e-4
    assert _rel(f.linear.weight.grad.cpu().numpy(), W64.grad.numpy()) <= 1e-4
    assert _rel(f.linear.bias.grad.cpu().numpy(), b64.grad.numpy()) <= 1e-4


def test_default_odefunc_is_unchanged(dev):
    """differentiable=False (the default): the same bits as ops.rhs, and an output that does not require grad."""
    import torch
    import scipy.sparse as sp
    from gnode import ops, synth
    from gnode.ode_nn_ngraph_sim import ODEfunc
    n, H = 100, 16
    rp, ci = synth.er_csr(n, 300, seed=2)
    A = sp.csr_matrix((np.ones(ci.shape[0]), ci, rp), shape=(n, n))
    f = ODEfunc(A, 0.2, 0.1, H, dev).to(dev)
    y, _ = FC.vjp_inputs(2 * n, H, seed=1, sample_rows=n)
    yt = torch.from_numpy(y).to(dev).requires_grad_(True)
    out = f(0.0, yt)
    assert not out.requires_grad
    assert torch.equal(out, ops.rhs(f.graph, yt.detach(), f.linear.weight.detach(), f.linear.bias.detach()))
    fd = ODEfunc(A, 0.2, 0.1, H, dev, differentiable=True).to(dev)
    fd.load_state_dict(f.state_dict())
    out_d = fd(0.0, yt)
    assert out_d.requires_grad and torch.equal(out_d.detach(), out)
    with torch.no_grad():
        assert not fd(0.0, yt).requires_grad
    # once_differentiable: a double backward is refused with a clear error
    g, = torch.autograd.grad(out_d.sum(), yt, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), yt)
