"""GPU: the training gradient on the REAL training graphs against float64 vectors the reference classes produced
(tests/golden/real_*.npz, tests/golden/make_golden_realgraphs.py; their oracle reproduction and the sensitivity of these
tolerances: test_real_graphs_golden.py).  Through the product's call surface, as the reference trains: the drop-in
ODEBlock, the fused get_sir_t_nodes subsample, the L1 loss op, loss.backward().

  * configs[4] (hidden 8, maxTime 20: 39 intervals) on batches of eight samples concatenated along the node axis:
    composition A (all five graphs, 24 410 rows) on the small-hidden persistent launch (k_persg / k_persg_bwd: one launch
    across ~190 workgroups with a flag barrier per step, hub segments in LDS) and on the per-step kernels; composition B
    (eight wiki-vote samples, 56 528 rows: more than one resident grid) on the per-step kernels (k_hub_seg / k_hub_reduce).
  * configs[1] / [2] (hidden 64, maxTime 30: 59 intervals) on fb-social and wiki-vote: the H = 64 persistent launch with
    its hub path (pers_hub_*), over kept activations and with the recomputing backward.
  * Monte-Carlo SIR on wiki-vote seeded at its 1 065-edge hub: bit-exact against the oracle's Philox restatement.
Tolerances: outputs 2e-5 of each tensor's max, loss 1e-6, gradients 2e-4 relative; the reference's own fp32 run of the same
rule ("G32:") is printed beside each GPU distance."""
import numpy as np
import pytest

import fixture_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-12)


def _check(tag, d, model, S, I, R, y, rows):
    """outputs at the kept rows, loss, loss.backward(), the 8 gradients; returns the gradient distances"""
    import torch
    from gnode import ops
    from gnode.autograd import l1_loss_sum
    maxTime = int(d["maxTime"])
    for c, got in zip("SIR", (S, I, R)):
        got = got.detach()[..., 0].double().cpu().numpy()[d["rows_kept"]]
        err = _rel(got, d[c])
        print(f"[{tag}] {c}: GPU vs reference float64 {err:.2e}; reference fp32 (max abs) {float(d['out32_err']):.2e}")
        assert err <= 2e-5, f"{c}: rel err {err:.2e}"
    loss = l1_loss_sum(S, I, R, torch.from_numpy(y).to(S.device), 1) / (rows * (maxTime - 1) * 3)
    assert abs(float(loss.detach()) - float(d["loss"])) <= 1e-6, (float(loss.detach()), float(d["loss"]))
    loss.backward()
    named = dict(model.named_parameters())
    for k in [k[2:] for k in d if k.startswith("G:")]:
        want = d["G:" + k]
        if k == "linearS2.bias":                                              # exact gradient 0 (softmax shift invariance)
            assert float(named[k].grad.abs().max()) <= 1e-6
            continue
        err = _rel(named[k].grad.cpu().numpy(), want)
        print(f"[{tag}] {k}: GPU vs reference float64 {err:.2e}; reference fp32 vs its float64 {_rel(d['G32:' + k], want):.2e}")
        assert err <= 2e-4, f"{k}: rel err {err:.2e}"


@pytest.mark.parametrize("persist", [True, False], ids=["default", "per_step"])
@pytest.mark.parametrize("name,kind", [(FC.MULTI[0], 3), (FC.MULTI[1], 0)], ids=["A", "B"])
def test_multi_graph_training_gradient_on_real_graphs(name, kind, persist, dev, monkeypatch):
    """configs[4] through gnode.ode_nn_ngraphs: the default path (A: small-hidden persistent, kind 3; B: per step, kind 0)
    and the per-step kernels (ops.PERSIST_DEFAULT off) against the reference's float64 run."""
    import torch
    from gnode import ops
    from gnode import ode_nn_ngraphs as multi
    monkeypatch.setattr(ops, "PERSIST_DEFAULT", persist)
    gs = FC.graphs()
    d = FC.load(name)
    x, P, y = FC.inputs(d, gs)
    H, maxTime, deltaT = int(d["H"]), int(d["maxTime"]), float(d["deltaT"])
    rows = x.shape[0]
    model = multi.ODEBlock(maxTime, deltaT, H, multi.ODEfunc([FC.adj(*rc) for rc in gs], H, dev), dev).to(dev)
    model.load_state_dict({**model.state_dict(), **{k: torch.from_numpy(v) for k, v in P.items()}})
    xt = torch.from_numpy(x).to(dev)
    rows_out = ops.subsample_rows(maxTime, deltaT)
    g = model.odefunc.graph_for(xt[:, 3 + 2])
    assert g.n == rows
    path = ops.forward_path(g, rows, H, len(ops.time_grid(maxTime, deltaT)) - 1, len(rows_out), want_sol=True)[0]
    print(f"[{name} {'default' if persist else 'per_step'}] rows {rows}: forward path kind {path}")
    assert path == (kind if persist else 0), path
    S, I, R = model(xt, out_rows=rows_out)
    if path == 3:
        assert ops.forward_status() == 0
    _check(f"{name} {'default' if persist else 'per_step'}", d, model, S, I, R, y, rows)
    if path == 3:
        assert ops.backward_status() == 0


@pytest.mark.parametrize("keep", [True, False], ids=["kept", "recompute"])
@pytest.mark.parametrize("name", FC.SINGLE)
def test_single_graph_training_gradient_on_real_graphs(name, keep, dev, monkeypatch):
    """configs[1] / [2] through gnode.ode_nn_ngraph_sim at B = 1, H = 64, the full 59-interval adjoint on the real
    topology: the persistent launch (kind 2) with hub rows, over kept activations and recomputing them."""
    import torch
    from gnode import ops
    from gnode.ode_nn_ngraph_sim import ODEBlock, ODEfunc
    monkeypatch.setattr(ops, "KEEP_DEFAULT", keep)
    gs = FC.graphs()
    d = FC.load(name)
    x, P, y = FC.inputs(d, gs)
    rp, ci = gs[int(d["graph"])]
    n, H, maxTime, deltaT = rp.shape[0] - 1, int(d["H"]), int(d["maxTime"]), float(d["deltaT"])
    assert int((np.diff(rp) > 96).sum()) > 0                                 # hub rows (GN_HUB_T = 96)
    model = ODEBlock(maxTime, deltaT, n, [0], H, ODEfunc(FC.adj(rp, ci), 0.2, 0.1, H, dev), dev).to(dev)
    model.load_state_dict({**model.state_dict(), **{k: torch.from_numpy(v) for k, v in P.items()}})
    rows_out = ops.subsample_rows(maxTime, deltaT)
    path = ops.forward_path(model.odefunc.graph, n, H, len(ops.time_grid(maxTime, deltaT)) - 1, len(rows_out), want_sol=True)[0]
    print(f"[{name} {'kept' if keep else 'recompute'}] forward path kind {path}")
    assert path == 2, path
    S, I, R = model(torch.from_numpy(x).to(dev), out_rows=rows_out)
    assert ops.forward_status() == 0
    _check(f"{name} {'kept' if keep else 'recompute'}", d, model, S, I, R, y, n)
    assert ops.backward_status() == 0


def test_sir_philox_on_wikivote_bit_exact_vs_oracle(dev):
    """test_sir_philox_bit_exact_vs_oracle's contract on real wiki-vote (its "hubs" case is a Chung-Lu stand-in): 64
    sims, T = 20, seeded at the 1 065-edge hub and a low-degree node."""
    import gnode_oracle as O
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import sir_counts
    rp, ci = FC.graphs()[FC.WIKI]
    n, deg = rp.shape[0] - 1, np.diff(rp)
    hub = int(np.argmax(deg))
    assert deg[hub] == 1065
    seeds, sims, T = [hub, int(np.argmin(deg))], 64, 20
    got = sir_counts(DeviceGraph(rp, ci), seeds, 0.3, 0.2, sims, T, rng_seed=0xABCDEF0123, sim_offset=11).cpu().numpy().astype(np.uint32)
    want = O.sir_philox(n, rp, ci, seeds, 0.3, 0.2, sims, T, rng_seed=0xABCDEF0123, sim_offset=11)
    assert np.array_equal(got, want)
    assert np.array_equal(got[0, 1:] + got[1, 1:] + got[2, 1:], np.full((T - 1, n), sims, np.uint32))
    assert int(got[2, -1].sum()) > 0                                          # the epidemic took off from the hub
