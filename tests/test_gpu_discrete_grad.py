"""GPU: the exact gradient of the Euler solve, ODEBlock(adjoint=False) (include/gnode.h gnode_backward_discrete_f32; DESIGN
section 7.3).  Held to float64 vectors of the reference's own classes under a differentiable Euler loop (tests/golden/
discrete_*.npz), to the float64 restatement (oracle/gnode_restate.py exact_grads) over H = 4 .. 128, hub graphs, 75k x 4 and 2- / 3-point
grids, and to autograd through a Python Euler loop of ODEfunc(differentiable=True) on the GPU.  Then the call-level contract:
deterministic, capturable, parameter gradients unchanged by gx, keep-produced trajectories refused, RK4 refused, and training
with it (Adam, the drop-in script under GNODE_ADJOINT=0) works."""
import os

import numpy as np
import pytest

import fixture_cases as FC
import gnode_oracle as O
import gnode_restate as RS
from gnode_restate import KEYS

pytestmark = pytest.mark.gpu

CASES = ["discrete_karate_B2_H64_T20", "discrete_loops40_B3_H8_T5", "discrete_er200_B2_H48_T6",
         "discrete_er200_B2_H128_T4", "discrete_fbsocial_B1_H64_T30", "discrete_multi8_H8_T20"]
TOL = 2e-4


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _exact_case(name, dev):
    """_case of the input-gradient tests (the same inputs) with the model switched to adjoint=False"""
    d, model, xt, y = FC.gpu_case(name, dev)
    model.adjoint = False
    return d, model, xt, y


def _check(got, want, label, tol=TOL):
    """got: {key: tensor / array}, want: {key: float64 array}; max-abs error over the gradient's max-abs, with a floor at 1e-3 of
    the overall scale; linearS2.bias (exactly 0: softmax is shift invariant) is held to the overall scale"""
    scale = max(float(np.abs(want[k]).max()) for k in want)
    for k, w in want.items():
        g = got[k].detach().double().cpu().numpy() if hasattr(got[k], "detach") else np.asarray(got[k], dtype=np.float64)
        g = g.reshape(w.shape)
        if k == "linearS2.bias":
            assert float(np.abs(g).max()) <= 1e-4 * scale, (label, k, g)
            continue
        err = float(np.abs(g - w).max()) / max(float(np.abs(w).max()), 1e-3 * scale)
        assert err <= tol, (label, k, err)


@pytest.mark.parametrize("fused", [True, False], ids=["out_rows", "full_grid"])
@pytest.mark.parametrize("name", CASES)
def test_exact_gradient_matches_reference(name, fused, dev):
    d, model, xt, y = _exact_case(name, dev)
    xt.requires_grad_(True)
    loss = FC.gpu_loss(d, model, xt, y, fused)
    assert abs(float(loss.detach()) - float(d["loss"])) <= 1e-6
    loss.backward()
    named = dict(model.named_parameters())
    got = {k: named[k].grad for k in KEYS}
    want = {k: d["G:" + k] for k in KEYS}
    for k in KEYS:              # tolerance: 2e-4, or 4x the reference's own fp32 distance where that is larger (never, today)
        if k != "linearS2.bias":
            yard = float(np.abs(d["G32:" + k] - d["G:" + k]).max()) / float(np.abs(d["G:" + k]).max())
            assert 4 * yard <= TOL, (k, yard)
    _check(got, want, name)
    gx = xt.grad.detach().double().cpu().numpy().reshape(-1, xt.shape[-1])
    err = float(np.abs(gx[:, :5] - d["G:x"]).max()) / float(np.abs(d["G:x"]).max())
    print(f"[{name}] x.grad {err:.2e}")
    assert err <= TOL, err
    assert float(np.abs(gx[:, 5:]).max()) == 0.0


def _ops(graph, x2d, params, dts, out_rows, gS, gI, gR, **kw):
    from gnode import ops
    return ops.backward(graph, x2d, params, dts, "euler", out_rows, kw.pop("sol"), gS, gI, gR, adjoint=False, **kw)


def _setup(rp, ci, B, H, dts, out_rows, dev, seed=0):
    """(graph, x2d, params, sol, gS, gI, gR as torch, P, x2d numpy, gS.. numpy) of a forward without keep"""
    import torch
    from gnode import ops
    from gnode.graph import DeviceGraph
    sy = FC.synth()
    n = rp.shape[0] - 1
    P = sy.linear_params(H, seed=seed)
    x = sy.samples(n, B, H, seed=seed + 1).reshape(B * n, -1)
    g = DeviceGraph(rp, ci)
    params = {k: torch.from_numpy(v).to(dev).contiguous() for k, v in P.items()}
    x2d = torch.from_numpy(x).to(dev)
    S, I, R, sol = ops.forward(g, x2d, params, dts, "euler", out_rows, want_sol=True, want_keep=False)
    rng = np.random.default_rng(seed + 2)
    gn = [rng.normal(size=tuple(S.shape)).astype(np.float32) for _ in range(3)]
    gt = [torch.from_numpy(a).to(dev) for a in gn]
    return g, x2d, params, sol, gt, P, x, gn


GRIDS = {"T6": (np.full(11, 0.5, np.float32), np.arange(0, 12, 2, dtype=np.int32)),
         "3pt": (np.asarray([0.5, 0.5], np.float32), None), "2pt": (np.asarray([0.5], np.float32), None)}


@pytest.mark.parametrize("grid", ["T6", "3pt", "2pt"])
@pytest.mark.parametrize("graph", ["er", "chung_lu"])
@pytest.mark.parametrize("H", [4, 8, 16, 24, 32, 48, 64, 128])
def test_exact_gradient_matches_restatement(H, graph, grid, dev):
    dts, out_rows = GRIDS[grid]
    if graph == "er":
        rp, ci, _ = O.er_graph(400, 1600, seed=H)
    else:
        rp, ci, _ = O.chung_lu_graph(1500, 9000, seed=H)
        assert int(np.diff(rp).max()) > 96                     # rows above the hub threshold (GN_HUB_T)
    g, x2d, params, sol, (gS, gI, gR), P, x, gn = _setup(rp, ci, 2, H, dts, out_rows, dev, seed=H)
    got = _ops(g, x2d, params, dts, out_rows, gS, gI, gR, sol=sol, want_x=True)
    want = RS.exact_grads(x, P, (rp, ci), dts, RS.linear_loss(*gn, out_rows))
    wx = want.pop("x")
    _check(got, want, (H, graph, grid))
    err = float(np.abs(got["x"].double().cpu().numpy()[:, :5] - wx[:, :5]).max()) / float(np.abs(wx[:, :5]).max())
    assert err <= TOL, err


def test_exact_gradient_75k_by_4(dev):
    """the large-graph H = 64 shape (many workgroups, XCD-affine tile queues), 3-point grid"""
    sy = FC.synth()
    rp, ci = sy.er_csr(75000, 300000, seed=1)
    dts, out_rows = GRIDS["3pt"]
    g, x2d, params, sol, (gS, gI, gR), P, x, gn = _setup(rp, ci, 4, 64, dts, out_rows, dev, seed=7)
    got = _ops(g, x2d, params, dts, out_rows, gS, gI, gR, sol=sol, want_x=True)
    want = RS.exact_grads(x, P, (rp, ci), dts, RS.linear_loss(*gn, out_rows))
    wx = want.pop("x")
    _check(got, want, "75k x 4")
    err = float(np.abs(got["x"].double().cpu().numpy()[:, :5] - wx[:, :5]).max()) / float(np.abs(wx[:, :5]).max())
    assert err <= TOL, err


@pytest.mark.parametrize("H", [8, 64])
def test_matches_autograd_through_a_python_euler_loop(H, dev):
    """ODEBlock(adjoint=False) against torch autograd through y += dt * ODEfunc(differentiable=True)(t, y) on the GPU: the
    same gradient by another road (one autograd node and one RHS VJP per step)"""
    import torch
    from gnode.ode_nn_ngraph_sim import ODEBlock, ODEfunc
    rp, ci, _ = O.er_graph(200, 700, seed=3)
    n, B, maxTime, deltaT = 200, 2, 6, 0.5
    sy = FC.synth()
    P = sy.linear_params(H, seed=11)
    f = ODEfunc(FC.adj(rp, ci), 0.2, 0.1, H, dev, differentiable=True)
    model = ODEBlock(maxTime, deltaT, n, [0], H, f, dev, adjoint=False).to(dev)
    model.load_state_dict({**model.state_dict(), **{k: torch.from_numpy(v) for k, v in P.items()}})
    x = torch.from_numpy(sy.samples(n, B, H, seed=12)).to(dev)
    w = torch.randn((3, model._dts.shape[0] + 1, B * n), generator=torch.Generator().manual_seed(1)).to(dev)

    def loss_of(S, I, R):
        return (S.reshape(w[0].shape) * w[0]).sum() + (I.reshape(w[1].shape) * w[1]).sum() + (R.reshape(w[2].shape) * w[2]).sum()

    xa = x.clone().requires_grad_(True)
    loss_of(*model(xa)).backward()
    fast = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    fast["x"] = xa.grad.clone()
    model.zero_grad(set_to_none=True)
    xb = x.clone().requires_grad_(True)
    x2 = xb.reshape(-1, xb.shape[-1])
    enc = lambda s: torch.relu(model.linearS1(s.unsqueeze(-1)))
    y = torch.cat((enc(x2[:, 0]), enc(x2[:, 1]), enc(x2[:, 2]), x2[:, 3:]))
    sol = [y]
    for k, dt in enumerate(model._dts):
        sol.append(sol[-1] + float(dt) * f(k, sol[-1]))
    sol = torch.stack(sol)
    q = B * n
    ro = lambda Y: model.linearS2(torch.relu(model.linear3(Y)))
    out = torch.softmax(torch.cat((ro(sol[:, :q]), ro(sol[:, q:2 * q]), ro(sol[:, 2 * q:3 * q])), -1), 2)
    loss_of(out[..., 0], out[..., 1], out[..., 2]).backward()
    slow = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    slow["x"] = xb.grad
    assert set(fast) == set(slow)
    want = {k: v.detach().double().cpu().numpy() for k, v in slow.items()}
    want["x"] = want["x"][..., :5]
    fast["x"] = fast["x"][..., :5]
    _check(fast, want, ("python loop", H), tol=1e-4)


@pytest.mark.parametrize("case", ["h64", "h8", "h48"])
def test_repeatable_capturable_and_gx_free(case, dev):
    """two calls agree bitwise; a torch.cuda.graph capture replays to the eager bits; the parameter gradients do not depend
    on whether gx is asked for"""
    import torch
    H = {"h64": 64, "h8": 8, "h48": 48}[case]
    rp, ci = FC.synth().heavy_tail_csr(900, 5000, seed=2)
    dts, out_rows = np.full(11, 0.5, np.float32), np.arange(0, 12, 2, dtype=np.int32)
    g, x2d, params, sol, (gS, gI, gR), *_ = _setup(rp, ci, 3, H, dts, out_rows, dev, seed=21)
    run = lambda **kw: _ops(g, x2d, params, dts, out_rows, gS, gI, gR, sol=sol, **kw)
    a, b = run(want_x=True), run(want_x=True)
    c = run()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    assert torch.equal(a["x"], b["x"])
    run(want_x=True)                                   # warm-up on the capture stream's allocator
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = run(want_x=True)
    graph.replay()
    torch.cuda.synchronize()
    for k in list(KEYS) + ["x"]:
        assert torch.equal(cap[k], a[k]), k


def test_keep_trajectory_and_rk4_are_refused(dev):
    import torch
    from gnode import _lib, ops
    from gnode.ode_nn_ngraph_sim import ODEBlock, ODEfunc
    rp, ci, _ = O.er_graph(300, 1200, seed=5)
    dts = np.full(11, 0.5, np.float32)
    sy = FC.synth()
    P = sy.linear_params(64, seed=1)
    from gnode.graph import DeviceGraph
    g = DeviceGraph(rp, ci)
    params = {k: torch.from_numpy(v).to(dev) for k, v in P.items()}
    x2d = torch.from_numpy(sy.samples(300, 2, 64, seed=2).reshape(600, -1)).to(dev)
    S, I, R, sol = ops.forward(g, x2d, params, dts, "euler", None, want_sol=True, want_keep=True, persist=False)
    assert sol.gnode_keep is not None and sol.gnode_info & 2
    one = torch.ones_like(S)
    with pytest.raises(_lib.GnodeError, match="keep"):
        ops.backward(g, x2d, params, dts, "euler", None, sol, one, one, one, adjoint=False)
    with pytest.raises(_lib.GnodeError, match="Euler only"):
        ops.backward(g, x2d, params, dts, "rk4", None, sol, one, one, one, adjoint=False)
    with pytest.raises(_lib.GnodeError, match="Euler only"):
        ODEBlock(6, 0.5, 300, [0], 64, ODEfunc(FC.adj(rp, ci), 0.2, 0.1, 64, dev), dev, method="rk4", adjoint=False)


def test_default_is_the_adjoint(dev):
    """ODEBlock() keeps the adjoint gradient bit for bit; adjoint=False gives a different one"""
    import torch
    d, model, xt, y = FC.gpu_case("input_grad_fbsocial_B1_H64_T30", dev)
    assert model.adjoint is True
    grads = []
    for adjoint in (True, True, False):
        model.adjoint = adjoint
        model.zero_grad(set_to_none=True)
        FC.gpu_loss(d, model, xt, y, True).backward()
        grads.append(model.odefunc.linear.weight.grad.clone())
    assert torch.equal(grads[0], grads[1]) and not torch.equal(grads[0], grads[2])


def test_adam_lowers_the_loss(dev):
    import torch
    d, model, xt, y = _exact_case("discrete_karate_B2_H64_T20", dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        loss = FC.gpu_loss(d, model, xt, y, True)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("adam:", losses[0], "->", losses[-1])
    assert losses[-1] < 0.9 * losses[0]


def test_drop_in_script_trains_with_exact_gradients(tmp_path, monkeypatch, dev):
    """two epochs of the single-graph drop-in with the trainer's knob off (what GNODE_ADJOINT=0 sets at import), under its
    HIP-graph replay: the exact backward runs and the CSV row is written"""
    import pandas as pd
    from gnode import ops, trainer
    monkeypatch.setattr(trainer, "ADJOINT_DEFAULT", False)
    calls = []
    real = ops._backward_discrete
    monkeypatch.setattr(ops, "_backward_discrete", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.chdir(tmp_path)
    os.makedirs("real_graphs"); os.makedirs("multi-graph-1/Experiments-seed2-toy")
    G = FC.mk_graph("real_graphs/toy.pkl", 80, 240, 1)
    n = G.number_of_nodes()
    rng = np.random.default_rng(0)
    seeds = [sorted(rng.choice(n, 2, replace=False).tolist()) for _ in range(10)]
    argv = ["--lr", "0.01", "--epochs", "2", "--hidden", "64", "--I_indices"] + [str(s) for s in seeds] + \
           ["--beta"] + [f"{b:.3f}" for b in rng.uniform(0.1, 0.5, 10)] + ["--gamma"] + [f"{g:.3f}" for g in rng.uniform(0.1, 0.5, 10)] + \
           ["--deltaT", "0.5", "--maxTime", "8", "--sim", "200", "--trial", "0", "--dataset", "./real_graphs/toy",
            "--path_to_save", "./multi-graph-1/Experiments-seed2-toy", "--batch_size", "4",
            "--train_val_test_ratio", "0.6", "0.2", "0.2", "--model", "ode_nn"]
    assert trainer.main_single(argv) == 0
    assert calls, "the exact backward never ran"
    df = pd.read_csv("multi-graph-1/Experiments-seed2-toy/Metrics-trials-toy")
    assert len(df) == 1 and df["model"][0] == "ode_nn" and np.isfinite(df["test_loss"][0]) and df["test_loss"][0] < 0.5
