"""GPU: the ODEBlock input gradient x.grad (include/gnode.h gnode_backward_dx_f32 / gnode_backward_rk4_dx_f32) against
float64 vectors the reference classes produced (tests/golden/input_grad_*.npz, make_golden_input_grad.py; the spec they
pin: oracle/gnode_restate.py, test_input_grad_golden.py), through the drop-in ODEBlocks, loss.backward() as the reference
takes it.  Per column group ({S0, I0, R0} and {beta, gamma}) the max-abs error over the group's max-abs is held to
max(2e-4, 4 x the reference's own fp32 distance).  Then the call-level contract: parameter gradients unchanged bit for bit,
gx = NULL is the old call, two calls agree bitwise, keep + gx is refused, and one descent step on beta / gamma helps."""
import numpy as np
import pytest

import fixture_cases as FC

pytestmark = pytest.mark.gpu

CASES = ["input_grad_karate_B2_H64_T20", "input_grad_loops40_B3_H8_T5", "input_grad_er200_B2_H48_T6",
         "input_grad_er200_B2_H128_T4", "input_grad_fbsocial_B1_H64_T30", "input_grad_multi8_H8_T20",
         "input_grad_rk4_karate_B2_H64_T20"]


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _group_errors(d, gx):
    got = gx.detach().double().cpu().numpy().reshape(-1, gx.shape[-1])
    want = d["GX"]
    errs = [float(np.abs(got[:, c] - want[:, c]).max() / np.abs(want[:, c]).max()) for c in (slice(0, 3), slice(3, 5))]
    return errs, float(np.abs(got[:, 5:]).max())


@pytest.mark.parametrize("persist", [True, False], ids=["persist", "per_step"])
@pytest.mark.parametrize("fused", [True, False], ids=["out_rows", "full_grid"])
@pytest.mark.parametrize("trainable", [True, False], ids=["trainable", "frozen"])
@pytest.mark.parametrize("name", CASES)
def test_input_grad_matches_reference(name, trainable, fused, persist, dev, monkeypatch):
    from gnode import ops
    monkeypatch.setattr(ops, "PERSIST_DEFAULT", persist)
    d, model, xt, y = FC.gpu_case(name, dev)
    model.requires_grad_(trainable)
    xt.requires_grad_(True)
    loss = FC.gpu_loss(d, model, xt, y, fused)
    assert abs(float(loss.detach()) - float(d["loss"])) <= 1e-6, (float(loss.detach()), float(d["loss"]))
    loss.backward()
    assert xt.grad is not None
    (e0, e1), rest = _group_errors(d, xt.grad)
    tol = [max(2e-4, 4 * float(v)) for v in d["yard32"]]
    print(f"[{name}] S0/I0/R0 {e0:.2e} (tol {tol[0]:.1e}), beta/gamma {e1:.2e} (tol {tol[1]:.1e})")
    assert e0 <= tol[0] and e1 <= tol[1], (e0, e1, tol)
    assert rest == 0.0
    named = dict(model.named_parameters())
    for k in ops.PARAM_KEYS:                                           # (the drop-in's unused LayerNorm never gets one)
        assert (named[k].grad is not None) == trainable, k


def _ops_call(name, dev, persist=False):
    """(run) for the call-level tests: run(**kw) -> ops.backward's dict on one forward's trajectory (want_keep=False)"""
    import torch
    from gnode import ops
    d, model, xt, y = FC.gpu_case(name, dev)
    params = {k: v.detach().contiguous() for k, v in model.state_dict().items() if k in ops.PARAM_KEYS}
    x2d = xt.reshape(-1, xt.shape[-1]).contiguous()
    dts = ops.step_sizes(ops.time_grid(int(d["maxTime"]), float(d["deltaT"])))
    rows_out = ops.subsample_rows(int(d["maxTime"]), float(d["deltaT"]))
    graph = model.odefunc.graph if "picks" not in d else model.odefunc.graph_for(x2d[:, 5])
    method = str(d["method"])
    S, I, R, sol = ops.forward(graph, x2d, params, dts, method, rows_out, want_sol=True, want_keep=False, persist=persist)
    g = torch.Generator().manual_seed(5)
    gS, gI, gR = (torch.randn(S.shape, generator=g).to(dev) for _ in range(3))
    return lambda **kw: ops.backward(graph, x2d, params, dts, method, rows_out, sol, gS, gI, gR, persist=persist, **kw)


RECOMPUTE = ["input_grad_loops40_B3_H8_T5", "input_grad_er200_B2_H48_T6", "input_grad_er200_B2_H128_T4",
             "input_grad_fbsocial_B1_H64_T30", "input_grad_multi8_H8_T20", "input_grad_rk4_karate_B2_H64_T20"]


@pytest.mark.parametrize("name", RECOMPUTE)
def test_params_bitwise_and_repeatable(name, dev):
    """On the recomputing path both calls take, gnode_backward_dx_f32's parameter gradients are gnode_backward_f32's bit
    for bit, and two gx calls agree bit for bit (no atomics); want_params=False returns the same gx alone."""
    import torch
    from gnode import ops
    run = _ops_call(name, dev)
    old = run(keep=None)
    new = run(keep=None, want_x=True)
    again = run(keep=None, want_x=True)
    only_x = run(keep=None, want_x=True, want_params=False)
    torch.cuda.synchronize()
    for k in ops.PARAM_KEYS:
        assert torch.equal(old[k], new[k]), k
        assert torch.equal(new[k], again[k]), k
    assert torch.equal(new["x"], again["x"]) and torch.equal(new["x"], only_x["x"])
    assert set(only_x) == {"x"}


@pytest.mark.parametrize("name", ["input_grad_fbsocial_B1_H64_T30", "input_grad_er200_B2_H48_T6",
                                  "input_grad_rk4_karate_B2_H64_T20"])
def test_null_gx_is_the_old_call(name, dev, monkeypatch):
    """gnode_backward_dx_f32 / gnode_backward_rk4_dx_f32 with gx = NULL are the old entry points, bit for bit."""
    import torch
    from gnode import _lib, ops
    run = _ops_call(name, dev, persist=None)
    old = run()
    real = _lib.load()

    class Dx:
        def __getattr__(self, a):
            return getattr(real, a)

        def gnode_backward_f32(self, *args):
            return real.gnode_backward_dx_f32(*args, None)

        def gnode_backward_rk4_f32(self, *args):
            return real.gnode_backward_rk4_dx_f32(*args, None)

    monkeypatch.setattr(_lib, "load", lambda: Dx())
    new = run()
    torch.cuda.synchronize()
    for k in ops.PARAM_KEYS:
        assert torch.equal(old[k], new[k]), k


def test_keep_with_gx_is_refused(dev):
    import torch
    from gnode import _lib, ops
    d, model, xt, y = FC.gpu_case("input_grad_fbsocial_B1_H64_T30", dev)
    params = {k: v.detach().contiguous() for k, v in model.state_dict().items() if k in ops.PARAM_KEYS}
    x2d = xt.reshape(-1, xt.shape[-1]).contiguous()
    dts = ops.step_sizes(ops.time_grid(int(d["maxTime"]), float(d["deltaT"])))
    rows_out = ops.subsample_rows(int(d["maxTime"]), float(d["deltaT"]))
    S, I, R, sol = ops.forward(model.odefunc.graph, x2d, params, dts, "euler", rows_out, want_sol=True, want_keep=True)
    assert sol.gnode_keep is not None
    g = torch.ones_like(S)
    with pytest.raises(_lib.GnodeError, match="keep"):
        ops.backward(model.odefunc.graph, x2d, params, dts, "euler", rows_out, sol, g, g, g, want_x=True)


def test_descent_on_beta_gamma_lowers_the_loss(dev):
    """Calibration as users run it: the model frozen, x.grad[..., 3:5] from one backward, one small step against it on an
    fb-social-size sample (Erdos-Renyi with fb-social's node and edge counts, 59 intervals) lowers the loss."""
    import torch
    from golden.labels import closed_form_labels
    from gnode import ops
    from gnode.ode_nn_ngraph_sim import ODEBlock, ODEfunc
    sy = FC.synth()
    n, H, maxTime, deltaT = 1893, 64, 30, 0.5
    rp, ci = sy.er_csr(n, 13835, seed=0)
    model = ODEBlock(maxTime, deltaT, n, [0], H, ODEfunc(FC.adj(rp, ci), 0.2, 0.1, H, dev), dev).to(dev)
    model.load_state_dict({**model.state_dict(), **{k: torch.from_numpy(v) for k, v in sy.linear_params(H, seed=3).items()}})
    model.requires_grad_(False)
    x = torch.from_numpy(sy.samples(n, 1, H, seed=7)).to(dev)
    y = closed_form_labels(1, n, maxTime).reshape(n, maxTime, 3)
    d = {"maxTime": maxTime, "deltaT": deltaT}
    xt = x.clone().requires_grad_(True)
    loss0 = FC.gpu_loss(d, model, xt, y, True)
    loss0.backward()
    g = xt.grad[..., 3:5]
    assert float(g.abs().max()) > 0
    step = 1e-2 * float(x[..., 3:5].abs().max()) / float(g.abs().max())
    x1 = x.clone()
    x1[..., 3:5] -= step * g
    with torch.no_grad():
        loss1 = FC.gpu_loss(d, model, x1, y, True)
    print(f"descent: loss {float(loss0):.9f} -> {float(loss1):.9f}")
    assert float(loss1) < float(loss0)
