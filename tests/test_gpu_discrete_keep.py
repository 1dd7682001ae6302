"""GPU: the exact gradient of the Euler solve on the forms of the training backward (include/gnode.h
gnode_backward_discrete_keep_f32, gnode_backward_discrete_path): over the forward's kept activations one
launch per interval (form 1), as one persistent H = 64 launch (form 2), as one persistent launch at H <= 32 (form 3).  Which
shape takes which form; against the reference's own classes under float64 (tests/golden/discrete_*.npz, 2e-4); against the
recomputing exact sweep (form 0, 1e-5 of each gradient's scale, the bar of test_gpu_persistent.py on its shape list); against
the float64 restatement on edge grids (2e-4); bitwise repeatable, capturable, give-up word 0."""
import os

import numpy as np
import pytest

import fixture_cases as FC
import gnode_oracle as O
import gnode_restate as RS
from gnode_restate import KEYS

pytestmark = pytest.mark.gpu
TOL = 2e-4


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _err(got, want):
    """per key: max-abs error over the gradient's max-abs, floored at 1e-3 of the overall scale (linearS2.bias, exactly 0 by
    softmax's shift invariance, over the overall scale): the measure of test_gpu_discrete_grad.py"""
    scale = max(float(np.abs(want[k]).max()) for k in want)
    out = {}
    for k, w in want.items():
        g = got[k].detach().double().cpu().numpy() if hasattr(got[k], "detach") else np.asarray(got[k], dtype=np.float64)
        g = g.reshape(w.shape)
        out[k] = float(np.abs(g).max()) / scale if k == "linearS2.bias" else \
            float(np.abs(g - w).max()) / max(float(np.abs(w).max()), 1e-3 * scale)
    return out


def _check(got, want, label, tol=TOL):
    errs = _err(got, want)
    print(f"[{label}] " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= (1e-4 if k == "linearS2.bias" else tol), (label, k, v)


def _spy(monkeypatch):
    """record the form (gnode_backward_discrete_path) and the keep argument of every exact backward the bridge makes"""
    from gnode import ops
    seen = []
    real = ops._backward_discrete

    def spy(graph, x2d, params, dts, out_rows, sol, *a, **k):
        seen.append((ops.discrete_path(graph, x2d.shape[0], x2d.shape[1] - 3, len(dts), out_rows, sol, k.get("keep"),
                                       k.get("persist"), k.get("want_x", False)), k.get("keep") is not None))
        return real(graph, x2d, params, dts, out_rows, sol, *a, **k)

    monkeypatch.setattr(ops, "_backward_discrete", spy)
    return seen


# ---- 2 + 4: paths of the reference-class fixtures through ODEBlock(adjoint=False), and their gradients under float64
@pytest.mark.parametrize("persist", [True, False], ids=["default", "persist_off"])
@pytest.mark.parametrize("name, form", [("discrete_fbsocial_B1_H64_T30", 2), ("discrete_multi8_H8_T20", 3),
                                        ("discrete_karate_B2_H64_T20", 0)])
def test_reference_class_gradients_and_paths(name, form, persist, dev, monkeypatch):
    from gnode import ops
    monkeypatch.setattr(ops, "PERSIST_DEFAULT", persist)
    seen = _spy(monkeypatch)
    d, model, xt, y = FC.gpu_case(name, dev)
    model.adjoint = False
    loss = FC.gpu_loss(d, model, xt, y, True)
    assert abs(float(loss.detach()) - float(d["loss"])) <= 1e-6
    loss.backward()
    want_form = form if persist else {2: 1, 3: 0, 0: 0}[form]
    # forms 1 / 2: the bridge passes the kept activations explicitly; form 0: it ran the forward without any
    assert seen == [(want_form, want_form in (1, 2))], seen
    assert ops.backward_status() == 0
    named = dict(model.named_parameters())
    _check({k: named[k].grad for k in KEYS}, {k: d["G:" + k] for k in KEYS}, (name, "persist" if persist else "per-interval"))


def _setup(rp, ci, B, H, dts, out_rows, dev, seed=0, want_keep=None, persist=None):
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
    S, I, R, sol = ops.forward(g, x2d, params, dts, "euler", out_rows, want_sol=True, want_keep=want_keep, persist=persist)
    rng = np.random.default_rng(seed + 2)
    gn = [rng.normal(size=tuple(S.shape)).astype(np.float32) for _ in range(3)]
    gt = [torch.from_numpy(a).to(dev) for a in gn]
    return g, x2d, params, sol, gt, P, x, gn


def _f64(x, P, csr, dts, gn, out_rows):
    """the float64 restatement's parameter gradients (oracle/gnode_restate.py exact_grads)"""
    want = RS.exact_grads(x, P, csr, dts, RS.linear_loss(*gn, out_rows))
    want.pop("x")
    return want


def _exact(g, x2d, params, dts, out_rows, sol, gt, **kw):
    from gnode import ops
    return ops.backward(g, x2d, params, dts, "euler", out_rows, sol, *gt, adjoint=False, **kw)


def test_synthetic_paths(dev):
    """form 1 above the persistent limit and with persist=False; form 0 for gx, for a trajectory without keep, for 2-point
    grids; form 3 / 0 at H = 8"""
    from gnode import ops
    from gnode.graph import DeviceGraph
    dts = np.full(11, 0.5, np.float32)
    some = object()
    big = DeviceGraph(*FC.synth().er_csr(20000, 80000, seed=1))               # 20 000 rows > 16 384
    assert ops.forward_path(big, 20000, 64, 11, want_sol=True)[0] == 0
    assert ops.discrete_path(big, 20000, 64, 11, keep=some) == 1
    mid = DeviceGraph(*FC.synth().er_csr(600, 2400, seed=1))
    assert ops.discrete_path(mid, 1200, 64, 11, keep=some) == 2
    assert ops.discrete_path(mid, 1200, 64, 11, keep=some, persist=False) == 1
    assert ops.discrete_path(mid, 1200, 64, 11, keep=None) == 0                 # want_keep=False
    assert ops.discrete_path(mid, 1200, 64, 11, keep=None, want_x=True) == 0
    assert ops.discrete_path(mid, 1200, 64, 11, keep=some, want_x=True) == 0    # (the call itself refuses keep with gx)
    assert ops.discrete_path(mid, 1200, 64, 1, keep=some) == 0                  # 2-point grid: nothing kept is of use
    assert ops.discrete_path(mid, 1200, 64, 2, keep=some) == 2
    assert ops.discrete_path(mid, 1200, 64, 2, out_rows=np.asarray([0, 1], np.int32), keep=some) == 1   # fold needs G >= 4
    assert ops.discrete_path(mid, 1200, 8, 11) == 3
    assert ops.discrete_path(mid, 1200, 8, 11, persist=False) == 0
    assert ops.discrete_path(mid, 1200, 8, 11, want_x=True) == 0
    assert ops.discrete_path(mid, 1200, 48, 11) == 0 and ops.discrete_path(mid, 1200, 128, 11) == 0


# ---- 3: an explicit keep on a keep-produced trajectory
def test_explicit_keep_returns_gradients(dev):
    import torch
    from gnode import _lib, ops
    rp, ci, _ = O.er_graph(300, 1200, seed=5)
    dts = np.full(11, 0.5, np.float32)
    g, x2d, params, sol, gt, P, x, gn = _setup(rp, ci, 2, 64, dts, None, dev, seed=1, want_keep=True, persist=False)
    assert sol.gnode_keep is not None and sol.gnode_info & 2
    got = _exact(g, x2d, params, dts, None, sol, gt, keep=sol.gnode_keep)
    _check(got, _f64(x, P, (rp, ci), dts, gn, None), "explicit keep")
    with pytest.raises(_lib.GnodeError, match="keep"):                          # "auto" passes no buffer
        _exact(g, x2d, params, dts, None, sol, gt)
    with pytest.raises(_lib.GnodeError, match="input gradient"):
        _exact(g, x2d, params, dts, None, sol, gt, keep=sol.gnode_keep, want_x=True)
    with pytest.raises(_lib.GnodeError, match="keep buffer"):                   # GNODE_ERR_WORKSPACE
        _exact(g, x2d, params, dts, None, sol, gt, keep=sol.gnode_keep[:1000])
    _, _, _, sol_n = ops.forward(g, x2d, params, dts, "euler", None, want_sol=True, want_keep=False)
    with pytest.raises(_lib.GnodeError, match="filled none"):
        _exact(g, x2d, params, dts, None, sol_n, gt, keep=sol.gnode_keep)


# ---- 5: against the recomputing exact sweep, on test_gpu_persistent.py's shapes
def _close(got, ref, label):
    for k in ref:
        scale = float((ref["linearS2.weight"] if k == "linearS2.bias" else ref[k]).abs().max()) + 1e-30
        err = float((got[k] - ref[k]).abs().max()) / scale
        assert err <= 1e-5, (label, k, err)


@pytest.mark.parametrize("n,m,B,launches,tail", [(1893, 13835, 1, 1, 0.0), (1893, 13835, 2, 1, 0.0), (1893, 13835, 8, 2, 0.0), (600, 2400, 5, 1, 0.0),
                                                 (7066, 100736, 1, 1, 0.0), (130, 500, 3, 1, 0.0), (1893, 13835, 1, 1, 0.8), (1893, 13835, 8, 2, 0.8),
                                                 (7066, 100736, 1, 1, 0.5)])
def test_h64_kept_and_persistent_match_recomputing(n, m, B, launches, tail, dev):
    import torch
    from gnode import ops, synth
    from gnode.graph import DeviceGraph
    rp, ci = synth.heavy_tail_csr(n, m, tail, seed=5) if tail else synth.er_csr(n, m, seed=5)
    g = DeviceGraph(rp, ci)
    P = {k: torch.from_numpy(v).to(dev) for k, v in synth.linear_params(64, seed=6).items()}
    x = torch.from_numpy(synth.samples(n, B, 64, seed=7)).to(dev).reshape(B * n, 67)
    maxTime, deltaT = 30, 0.5
    dts = ops.step_sizes(ops.time_grid(maxTime, deltaT))
    for rows_out in (ops.subsample_rows(maxTime, deltaT), None):                # last grid point not emitted (fold) / emitted
        T = len(rows_out) if rows_out is not None else len(dts) + 1
        gs = [torch.randn(T, B * n, device=dev) for _ in range(3)]
        _, _, _, sol_n = ops.forward(g, x, P, dts, "euler", rows_out, want_sol=True, want_keep=False)
        assert ops.discrete_path(g, B * n, 64, len(dts), rows_out, sol_n) == 0
        ref = _exact(g, x, P, dts, rows_out, sol_n, gs)
        _, _, _, sol = ops.forward(g, x, P, dts, "euler", rows_out, want_sol=True, want_keep=True)
        keep = sol.gnode_keep
        assert ops.discrete_path(g, B * n, 64, len(dts), rows_out, sol, keep) == 2
        assert ops.discrete_path(g, B * n, 64, len(dts), rows_out, sol, keep, persist=False) == 1
        kept = _exact(g, x, P, dts, rows_out, sol, gs, keep=keep, persist=False)
        pers = _exact(g, x, P, dts, rows_out, sol, gs, keep=keep, persist=True)
        assert ops.backward_status() == 0
        again = _exact(g, x, P, dts, rows_out, sol, gs, keep=keep, persist=True)
        _close(kept, ref, "kept")
        _close(pers, ref, "persistent")
        for k in ref:
            assert torch.equal(pers[k], again[k]), k


SMALL_H = [(22125, 250000, 1, 8, 0.0), (7066, 100736, 1, 8, 0.5), (1893, 13835, 3, 8, 0.8), (62, 159, 1, 8, 0.0), (300, 1500, 5, 8, 0.0),
           (7066, 100736, 1, 16, 0.5), (4000, 30000, 2, 16, 0.0), (1893, 13835, 2, 32, 0.8), (5000, 40000, 1, 32, 0.0)]


@pytest.mark.parametrize("n,m,B,H,tail", SMALL_H)
def test_small_hidden_persistent_matches_recomputing(n, m, B, H, tail, dev):
    import torch
    from gnode import ops, synth
    from gnode.graph import DeviceGraph
    rp, ci = synth.heavy_tail_csr(n, m, tail, seed=13) if tail else synth.er_csr(n, m, seed=13)
    g = DeviceGraph(rp, ci)
    P = {k: torch.from_numpy(v).to(dev) for k, v in synth.linear_params(H, seed=14).items()}
    x = torch.from_numpy(synth.samples(n, B, H, seed=15)).to(dev).reshape(B * n, 3 + H)
    maxTime, deltaT = 20, 0.5
    grids = [(ops.step_sizes(ops.time_grid(maxTime, deltaT)), ops.subsample_rows(maxTime, deltaT)),
             (np.asarray([0.5, 0.25, 1.0, 0.5, 0.125], dtype=np.float32), None)]
    for dts, rows_out in grids:
        T = len(rows_out) if rows_out is not None else len(dts) + 1
        gs = [torch.randn(T, B * n, device=dev) for _ in range(3)]
        _, _, _, sol = ops.forward(g, x, P, dts, "euler", rows_out, want_sol=True)
        assert ops.discrete_path(g, B * n, H, len(dts), rows_out, sol) == 3
        assert ops.discrete_path(g, B * n, H, len(dts), rows_out, sol, persist=False) == 0
        ref = _exact(g, x, P, dts, rows_out, sol, gs, persist=False)
        got = _exact(g, x, P, dts, rows_out, sol, gs, persist=True)
        assert ops.backward_status() == 0
        again = _exact(g, x, P, dts, rows_out, sol, gs, persist=True)
        _close(got, ref, (H, "persistent"))
        for k in ref:
            assert torch.equal(got[k], again[k]), k


# ---- 6: against float64
def test_large_hub_graph_on_the_kept_form(dev):
    """Chung-Lu, 20 000 rows (> 16 384: no persistent launch), rows above the hub threshold, 4 unequal steps"""
    from gnode import ops
    rp, ci, _ = O.chung_lu_graph(20000, 120000, seed=3)
    assert int(np.diff(rp).max()) > 96
    dts, out_rows = np.asarray([0.5, 0.25, 1.0, 0.5], np.float32), np.asarray([0, 2, 3], np.int32)
    g, x2d, params, sol, gt, P, x, gn = _setup(rp, ci, 1, 64, dts, out_rows, dev, seed=9)
    assert sol.gnode_keep is not None
    assert ops.discrete_path(g, 20000, 64, 4, out_rows, sol, sol.gnode_keep) == 1
    got = _exact(g, x2d, params, dts, out_rows, sol, gt, keep=sol.gnode_keep)
    _check(got, _f64(x, P, (rp, ci), dts, gn, out_rows), "chung-lu 20k, kept")


def _rows_variants(G):
    return {"all": None, "no_last": np.arange(G - 1, dtype=np.int32), "last_only": np.asarray([G - 1], np.int32),
            "ends": np.asarray(sorted({0, G - 2}), np.int32)}


@pytest.mark.parametrize("emit", ["all", "no_last", "last_only", "ends"])
@pytest.mark.parametrize("G", [2, 3, 4, 8])
@pytest.mark.parametrize("form", [1, 2, 3])
def test_edge_grids_match_float64(form, G, emit, dev):
    """2-, 3-, 4- and 8-point grids with unequal steps; the last grid point emitted and not (both fold variants); out_rows
    subsets; on a heavy-tailed graph with hub rows.  `form` is what the call asks for; short grids fall back as the plan says
    (asserted), and the gradient must be right whichever form runs"""
    from gnode import ops
    H = 8 if form == 3 else 64
    persist = form != 1
    rp, ci = FC.synth().heavy_tail_csr(1893, 13835, 0.8, seed=4)
    assert int(np.diff(rp).max()) > 96
    dts = np.asarray([0.5, 0.25, 1.0, 0.5, 0.125, 0.75, 0.5], np.float32)[:G - 1]
    out_rows = _rows_variants(G)[emit]
    g, x2d, params, sol, gt, P, x, gn = _setup(rp, ci, 2, H, dts, out_rows, dev, seed=G, persist=persist)
    keep = sol.gnode_keep
    assert (keep is not None) == (H == 64)
    path = ops.discrete_path(g, x2d.shape[0], H, G - 1, out_rows, sol, keep, persist)
    last_zero = out_rows is not None and int(out_rows[-1]) != G - 1
    if form == 3:
        assert path == 3
    elif G == 2:
        assert path == 0
    elif form == 2:
        assert path == (2 if G >= (4 if last_zero else 3) else 1)
    else:
        assert path == 1
    got = _exact(g, x2d, params, dts, out_rows, sol, gt, keep=keep, persist=persist)
    assert ops.backward_status() == 0
    _check(got, _f64(x, P, (rp, ci), dts, gn, out_rows), (form, G, emit, path))


# ---- 7: determinism and capture
@pytest.mark.parametrize("form", [1, 2, 3])
def test_repeatable_and_capturable(form, dev):
    import torch
    from gnode import ops
    H = 8 if form == 3 else 64
    persist = form != 1
    rp, ci = FC.synth().heavy_tail_csr(900, 5000, seed=2)
    dts, out_rows = np.full(11, 0.5, np.float32), np.arange(0, 12, 2, dtype=np.int32)
    g, x2d, params, sol, gt, *_ = _setup(rp, ci, 3, H, dts, out_rows, dev, seed=21, persist=persist)
    keep = sol.gnode_keep
    assert ops.discrete_path(g, x2d.shape[0], H, 11, out_rows, sol, keep, persist) == form
    run = lambda: _exact(g, x2d, params, dts, out_rows, sol, gt, keep=keep, persist=persist)
    a, b = run(), run()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                          # warm-up on the capture stream's allocator
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = run()
    for rep in range(4):
        for k in KEYS:
            cap[k].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert ops.backward_status() == 0, rep
        for k in KEYS:
            assert torch.equal(cap[k], a[k]), (rep, k)


def test_drop_in_script_trains_on_the_fast_sweeps(tmp_path, monkeypatch, dev):
    """two epochs of the single-graph drop-in with the trainer's knob off (GNODE_ADJOINT=0) under its HIP-graph replay: the
    exact backward runs over the kept activations, not on the recomputing form"""
    import pandas as pd
    from gnode import trainer
    monkeypatch.setattr(trainer, "ADJOINT_DEFAULT", False)
    seen = _spy(monkeypatch)
    monkeypatch.chdir(tmp_path)
    os.makedirs("real_graphs"); os.makedirs("multi-graph-1/Experiments-seed2-toy")
    G = FC.mk_graph("real_graphs/toy.pkl", 80, 240, 1)
    n = G.number_of_nodes()
    assert n > 64                                      # (not the one-workgroup forward, whose sweep stays recomputing)
    rng = np.random.default_rng(0)
    seeds = [sorted(rng.choice(n, 2, replace=False).tolist()) for _ in range(10)]
    argv = ["--lr", "0.01", "--epochs", "2", "--hidden", "64", "--I_indices"] + [str(s) for s in seeds] + \
           ["--beta"] + [f"{b:.3f}" for b in rng.uniform(0.1, 0.5, 10)] + ["--gamma"] + [f"{g:.3f}" for g in rng.uniform(0.1, 0.5, 10)] + \
           ["--deltaT", "0.5", "--maxTime", "8", "--sim", "200", "--trial", "0", "--dataset", "./real_graphs/toy",
            "--path_to_save", "./multi-graph-1/Experiments-seed2-toy", "--batch_size", "4",
            "--train_val_test_ratio", "0.6", "0.2", "0.2", "--model", "ode_nn"]
    assert trainer.main_single(argv) == 0
    assert seen and all(path == 2 and kept for path, kept in seen), seen
    df = pd.read_csv("multi-graph-1/Experiments-seed2-toy/Metrics-trials-toy")
    assert len(df) == 1 and np.isfinite(df["test_loss"][0]) and df["test_loss"][0] < 0.5
