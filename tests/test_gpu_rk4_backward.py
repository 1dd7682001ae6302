"""GPU: ODEBlock(method='rk4') trains -- the RK4 (3/8 rule) adjoint backward (gnode_backward_rk4_f32) against the
reference's classes under the restated torchdiffeq rule (tests/golden/make_golden_rk4_adjoint.py) and against the float64
restatement of oracle/gnode_restate.py."""
import numpy as np
import pytest

import gnode_restate as RS
from fixture_cases import rk4_case

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


def _model(dev, rp, ci, n, H, maxTime, deltaT, P):
    import torch
    import scipy.sparse as sp
    from gnode.ode_nn_ngraph_sim import ODEBlock, ODEfunc
    A = sp.csr_matrix((np.ones(ci.shape[0]), ci, rp), shape=(n, n))
    model = ODEBlock(maxTime, deltaT, n, [0], H, ODEfunc(A, 0.2, 0.1, H, dev), dev, method="rk4").to(dev)
    model.load_state_dict({**model.state_dict(), **{k: torch.from_numpy(v) for k, v in P.items()}})
    return model


@pytest.mark.parametrize("fused", [True, False], ids=["fused-subsample", "subsample-after"])
@pytest.mark.parametrize("name", ["rk4_adjoint_karate_H64_T20", "rk4_adjoint_loops40_H8_T5"])
def test_rk4_training_gradient_vs_reference_classes(name, fused, dev):
    import torch
    from gnode import ops
    from gnode.autograd import l1_loss_sum
    rp, ci, x, P, y, d = rk4_case(name)
    n, B, H, maxTime, deltaT = int(d["n"]), int(d["B"]), int(d["H"]), int(d["maxTime"]), float(d["deltaT"])
    model = _model(dev, rp, ci, n, H, maxTime, deltaT, P)
    xt = torch.from_numpy(x).to(dev)
    rows = ops.subsample_rows(maxTime, deltaT)
    if fused:
        S, I, R = model(xt, out_rows=rows)
    else:
        idx = torch.from_numpy(rows.astype(np.int64)).to(dev)
        S, I, R = (t[idx].contiguous() for t in model(xt))
    yt = torch.from_numpy(y).to(dev)
    loss = l1_loss_sum(S, I, R, yt, 1) / (B * n * (maxTime - 1) * 3)
    assert abs(float(loss.detach()) - float(d["loss"])) <= 1e-5
    loss.backward()
    named = dict(model.named_parameters())
    for k in P:
        if k == "linearS2.bias":                                # exact gradient 0 (softmax shift invariance)
            assert float(named[k].grad.abs().max()) <= 1e-6
            continue
        err = _rel(named[k].grad.cpu().numpy(), d["G:" + k])
        assert err <= 2e-4, f"{k}: rel err {err:.2e}"


@pytest.mark.parametrize("kind,n,m,B,H,maxTime,deltaT,sub", [
    ("er", 60, 200, 2, 8, 4, 0.5, False),
    ("er", 90, 300, 2, 32, 4, 0.25, False),
    ("er", 150, 700, 2, 64, 5, 0.5, True),
    ("er", 40, 100, 1, 128, 3, 0.5, False),
    ("cl", 600, 6000, 2, 64, 3, 0.5, False),                   # hub rows
    ("cl", 600, 6000, 2, 16, 3, 0.5, True),
    ("er", 33, 60, 2, 64, 0.5, 0.5, False),                    # one grid point (n_steps = 0): head + encoder only, no interval
    ("er", 33, 60, 2, 64, 1, 0.5, False),                      # two grid points: one interval
    ("er", 150, 700, 2, 64, 1.5, 0.5, True),                   # three grid points, subsampled: the last emits nothing
])
def test_rk4_param_grads_vs_restatement(kind, n, m, B, H, maxTime, deltaT, sub, dev):
    import torch
    import gnode_oracle as O
    from gnode import ops
    from gnode.graph import DeviceGraph
    rp, ci, _ = (O.er_graph if kind == "er" else O.chung_lu_graph)(n, m, seed=n + H)
    P = O.init_params(H, seed=H + 1)
    x = O.make_samples(n, B, H, seed=B)
    grid = O.time_grid(maxTime, deltaT)
    out_rows = ops.subsample_rows(maxTime, deltaT) if sub else None
    idx = out_rows if sub else np.arange(len(grid))
    rng = np.random.default_rng(0)
    gs = [rng.normal(size=(len(idx), B * n)).astype(np.float32) for _ in range(3)]
    want = RS.adjoint(x.reshape(B * n, 3 + H), P, (rp, ci), O.step_sizes(grid), RS.linear_loss(*gs, idx), "rk4")
    del want["x"]
    g = DeviceGraph(rp, ci)
    params = {k: torch.from_numpy(v).to(dev) for k, v in P.items()}
    x2d = torch.from_numpy(x).to(dev).reshape(B * n, 3 + H)
    dts = ops.step_sizes(grid)
    S, I, R, sol = ops.forward(g, x2d, params, dts, "rk4", out_rows, want_sol=True)
    gst = [torch.from_numpy(a).to(dev) for a in gs]
    got = ops.backward(g, x2d, params, dts, "rk4", out_rows, sol, *gst)
    again = ops.backward(g, x2d, params, dts, "rk4", out_rows, sol, *gst)
    # a gradient that is exactly 0 in this configuration (linearS2.bias always; linear3.bias when every head ReLU of a row is on
    # or off for all three compartments: softmax shift invariance) is fp32 rounding noise, held like linearS2.bias below
    scale = max(float(np.abs(w).max()) for w in want.values())
    for k in want:
        assert torch.equal(got[k], again[k]), f"{k}: not deterministic"
        if k == "linearS2.bias":
            continue
        if float(np.abs(want[k]).max()) <= 1e-9 * scale:
            assert float(got[k].abs().max()) <= 1e-4 * max(1.0, scale), k
            continue
        err = _rel(got[k].cpu().numpy(), want[k])
        assert err <= 2e-4, f"{k}: rel err {err:.2e}"
    assert abs(float(got["linearS2.bias"].cpu())) <= 1e-4 * max(1.0, float(np.abs(want["linearS2.weight"]).max()))


def test_rk4_adam_lowers_the_loss(dev):
    import torch
    from gnode import ops
    from gnode.autograd import l1_loss_sum
    rp, ci, x, P, y, d = rk4_case("rk4_adjoint_karate_H64_T20")
    n, B, H, maxTime, deltaT = int(d["n"]), int(d["B"]), int(d["H"]), int(d["maxTime"]), float(d["deltaT"])
    model = _model(dev, rp, ci, n, H, maxTime, deltaT, P)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    xt, yt = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    rows = ops.subsample_rows(maxTime, deltaT)
    losses = []
    for _ in range(15):
        opt.zero_grad()
        S, I, R = model(xt, out_rows=rows)
        loss = l1_loss_sum(S, I, R, yt, 1) / (B * n * (maxTime - 1) * 3)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses))
    assert losses[-1] < 0.95 * losses[0], losses
