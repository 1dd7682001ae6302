"""GPU: the drop-in entry points keep the reference's argv/file contract
(monitorer-sim.py:53-103 -> ode_nn_ngraph_sim.py:326-356; monitorer-ngraphs.py:49-87 ->
ode_nn_ngraphs.py:296-308).  Graph/label pickles here are written by the test itself."""
import os
import pickle

import numpy as np
import pytest

import fixture_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def test_single_graph_entry_point(tmp_path, monkeypatch, dev):
    import pandas as pd
    from gnode.trainer import main_single
    monkeypatch.chdir(tmp_path)
    os.makedirs("real_graphs"); os.makedirs("multi-graph-1/Experiments-seed2-toy")
    G = FC.mk_graph("real_graphs/toy.pkl", 80, 240, 1)
    n = G.number_of_nodes()
    rng = np.random.default_rng(0)
    seeds = [sorted(rng.choice(n, 2, replace=False).tolist()) for _ in range(10)]
    argv = ["--lr", "0.01", "--epochs", "3", "--hidden", "64", "--I_indices"] + [str(s) for s in seeds] + \
           ["--beta"] + [f"{b:.3f}" for b in rng.uniform(0.1, 0.5, 10)] + ["--gamma"] + [f"{g:.3f}" for g in rng.uniform(0.1, 0.5, 10)] + \
           ["--deltaT", "0.5", "--maxTime", "8", "--sim", "200", "--trial", "0", "--dataset", "./real_graphs/toy",
            "--path_to_save", "./multi-graph-1/Experiments-seed2-toy", "--batch_size", "4",
            "--train_val_test_ratio", "0.6", "0.2", "0.2", "--model", "ode_nn"]
    assert main_single(argv) == 0
    d = "multi-graph-1/Experiments-seed2-toy"
    assert pickle.load(open(d + "/initial-seed.pkl", "rb")) == seeds                      # ode_nn_ngraph_sim.py:353-356
    for s in seeds:
        for c in "SIR":
            a = pickle.load(open(f"{d}/toy-{c}-{s[0]}-{s[1]}.pkl", "rb"))                 # label cache naming :191-204
            assert a.shape == (8, n) and a.dtype == np.float64 and a.min() >= 0 and a.max() <= 1
    df = pd.read_csv(d + "/Metrics-trials-toy")
    assert list(df.columns)[:4] == ["trial", "model", "lr", "epochs"] and len(df) == 1 and df["model"][0] == "ode_nn"
    assert np.isfinite(df["test_loss"][0]) and df["test_loss"][0] < 0.5
    # second trial appends a row and reuses the label cache; with the mean-field comparison switched on
    # (the reference's `runge_kutta_baseline`, ode_nn_ngraph_sim.py:298-317, commented out there at :473)
    argv[argv.index("--trial") + 1] = "1"
    monkeypatch.setenv("GNODE_RK_BASELINE", "1")
    assert main_single(argv) == 0
    monkeypatch.delenv("GNODE_RK_BASELINE")
    df = pd.read_csv(d + "/Metrics-trials-toy")
    assert len(df) == 2 and df["loss_baseline"][0] == 0 and 0 < df["loss_baseline"][1] < 0.5 and df["rk_time"][1] > 0
    # the DMP comparison entry point on the same experiment directory (monitorer-sim.py:30-31 -> dmp.py)
    from gnode.trainer import main_dmp
    import io, contextlib
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert main_dmp(argv[:-1] + ["dmp"]) == 0
    line = [l for l in buf.getvalue().splitlines() if l.startswith("DMP baseline Loss")]
    assert len(line) == 1 and 0 < float(line[0].split(":")[1]) < 0.5
    # out-of-distribution split
    pickle.dump({"train": [0, 1, 2, 3, 4], "val": [5, 6], "test": [7, 8, 9]}, open(d + "/out-of-dist-gamma.pkl", "wb"))
    assert main_single(argv + ["--out_of_dist"]) == 0
    assert os.path.exists(d + "/Out-of-dist-gamma-toy") and os.path.exists(d + "/Out-of-dist-gamma-trials-toy")


def test_multi_graph_entry_point(tmp_path, monkeypatch, dev):
    import pandas as pd
    from gnode.trainer import main_multi
    from gnode.ode_nn import sir_torch
    monkeypatch.chdir(tmp_path)
    os.makedirs("real_graphs")
    names, sizes = ["ga", "gb", "gc"], [(40, 100), (70, 220), (55, 150)]
    ipg = [3, 3, 4]                                   # train: ga, gb ; val 2 + test 2 from gc
    rng = np.random.default_rng(3)
    for (name, (n, m)) in zip(names, sizes):
        G = FC.mk_graph(f"real_graphs/{name}.pkl", n, m, 5)
        d = f"multi-graph-1/Experiments-seed2-{name}"
        os.makedirs(d)
        k = max(ipg)
        seeds = [sorted(rng.choice(G.number_of_nodes(), 2, replace=False).tolist()) for _ in range(k)]
        betas, gammas = rng.uniform(0.1, 0.5, k).tolist(), rng.uniform(0.1, 0.5, k).tolist()
        pickle.dump(seeds, open(d + "/initial-seed.pkl", "wb"))
        pickle.dump(betas, open(d + "/initial-beta.pkl", "wb"))
        pickle.dump(gammas, open(d + "/initial-gamma.pkl", "wb"))
        for s, b, g in zip(seeds, betas, gammas):
            S, I, R = sir_torch(G, s, b, g, 100, 6)
            for c, a in zip("SIR", (S, I, R)):
                pickle.dump(a[0] / 100, open(f"{d}/{name}-{c}-{s[0]}-{s[1]}.pkl", "wb"))
    argv = ["--lr", "0.01", "--epochs", "2", "--hidden", "8", "--deltaT", "0.5", "--maxTime", "6", "--sim", "100",
            "--trial", "0", "--dataset", "./real_graphs/ga+gb+gc", "--path_to_save", "./multi-graph-1/Experiments-seed2-ga+gb+gc",
            "--batch_size", "2", "--train_val_test_ratio", "0.6", "0.2", "0.2", "--model", "ode_nn",
            "--instances_per_graph"] + [str(v) for v in ipg]
    os.makedirs("multi-graph-1/Experiments-seed2-ga+gb+gc")
    assert main_multi(argv) == 0
    df = pd.read_csv("multi-graph-1/Experiments-seed2-ga+gb+gc/Metrics-trials-ga+gb+gc")
    assert len(df) == 1 and np.isfinite(df["test_loss"][0])


def test_multi_graph_entry_point_from_empty_directory(tmp_path, monkeypatch, dev):
    """the multi-graph script from a CLEAN multi-graph-1/ (the reference ships karate's labels
    only and no epinions.pkl): `initial-*.pkl` sampled as monitorer-sim's random_parameters_SIR does, every label set
    generated with the Monte-Carlo kernel and written under the reference's names and conventions (probabilities;
    raw counts for wiki-vote, ode_nn_ngraphs.py:168-171), the missing graph pickle replaced by a synthetic stand-in;
    a second run finds everything in place and reuses it."""
    import pandas as pd
    from gnode.trainer import main_multi
    monkeypatch.chdir(tmp_path)
    os.makedirs("real_graphs")
    G1 = FC.mk_graph("real_graphs/ga.pkl", 40, 100, 5)
    G2 = FC.mk_graph("real_graphs/wiki-vote.pkl", 60, 200, 6)           # the name selects the raw-count convention
    ipg, sim, T = [2, 3, 4], 50, 5                                    # train: ga, wiki-vote ; val 2 + test 2 from epinions
    save = "./multi-graph-1/Experiments-seed2-ga+wiki-vote+epinions"
    os.makedirs(save)
    argv = ["--lr", "0.01", "--epochs", "2", "--hidden", "8", "--deltaT", "0.5", "--maxTime", str(T), "--sim", str(sim),
            "--trial", "0", "--dataset", "./real_graphs/ga+wiki-vote+epinions", "--path_to_save", save,
            "--batch_size", "2", "--train_val_test_ratio", "0.6", "0.2", "0.2", "--model", "ode_nn",
            "--standin", "90", "300", "--instances_per_graph"] + [str(v) for v in ipg]
    assert main_multi(argv) == 0
    dirs = {"ga": "multi-graph-1/Experiments-seed2-ga", "wiki-vote": "multi-graph-1/Experiments-gpu-seed2-wiki-vote",
            "epinions": "multi-graph-1/Experiments-seed2-epinions"}
    nodes = {"ga": G1.number_of_nodes(), "wiki-vote": G2.number_of_nodes(), "epinions": 90}
    stamp = {}
    for (name, d), k in zip(dirs.items(), ipg):
        seeds = pickle.load(open(d + "/initial-seed.pkl", "rb"))
        betas = pickle.load(open(d + "/initial-beta.pkl", "rb"))
        assert len(seeds) == k and all(len(s) == 2 and len(set(s)) == 2 for s in seeds)
        assert all(0.1 <= b <= 0.5 for b in betas)
        for s in seeds:
            arrs = [pickle.load(open(f"{d}/{name}-{c}-{s[0]}-{s[1]}.pkl", "rb")) for c in "SIR"]
            tot = arrs[0] + arrs[1] + arrs[2]
            assert arrs[0].shape == (T, nodes[name]) and arrs[0].dtype == np.float64
            if name == "wiki-vote":                                   # raw counts; the loader divides by sim
                assert np.all(tot[1:] == sim) and np.all(arrs[0] == np.round(arrs[0]))
            else:
                assert np.allclose(tot[1:], 1.0) and arrs[0].max() <= 1.0
            stamp[f"{d}/{name}-S-{s[0]}-{s[1]}.pkl"] = os.path.getmtime(f"{d}/{name}-S-{s[0]}-{s[1]}.pkl")
    df = pd.read_csv(save + "/Metrics-trials-ga+wiki-vote+epinions")
    assert len(df) == 1 and np.isfinite(df["test_loss"][0]) and np.isfinite(df["val_loss"][0])
    argv[argv.index("--trial") + 1] = "1"
    assert main_multi(argv) == 0                                      # everything is reused, nothing regenerated
    assert all(os.path.getmtime(p) == t for p, t in stamp.items())
    assert len(pd.read_csv(save + "/Metrics-trials-ga+wiki-vote+epinions")) == 2


def test_graph_replay_equals_eager(dev):
    """HIP-graph replay of (forward + L1 + adjoint backward) gives bit-identical training to eager launches."""
    import copy
    import torch
    import scipy.sparse as sp
    import gnode_oracle as O
    from gnode.ode_nn_ngraph_sim import ODEfunc, ODEBlock
    from gnode.trainer import Runner, sample_tensor
    n, H, maxTime = 90, 64, 6
    rp, ci, _ = O.er_graph(n, 300, seed=2)
    A = sp.csr_matrix((np.ones(ci.shape[0]), ci, rp), shape=(n, n))
    rng = np.random.default_rng(0)
    xs = [sample_tensor(n, H, sorted(rng.choice(n, 2, replace=False).tolist()), rng.uniform(0.1, 0.5), rng.uniform(0.1, 0.5))
          for _ in range(7)]
    ys = [torch.from_numpy(rng.dirichlet(np.ones(3), size=(n, maxTime))) for _ in range(7)]
    torch.manual_seed(0)
    base = ODEBlock(maxTime, 0.5, n, [0], H, ODEfunc(A, 0.2, 0.1, H, dev), dev).to(dev)
    hist = []
    for use_graphs in (False, True):
        model = copy.deepcopy(base)
        assert model.odefunc.graph is base.odefunc.graph
        torch.manual_seed(123)
        run = Runner(model, 1e-2, maxTime, 0.5, dev, stack=True, use_graphs=use_graphs)
        run.seed = 5
        losses = [run.train_epoch(xs, ys, 2, ep)[0] for ep in range(3)]       # batches of 2, last one of 1
        hist.append((losses, [p.detach().clone() for p in model.parameters()]))
    assert hist[0][0] == hist[1][0]
    assert all(torch.equal(a, b) for a, b in zip(hist[0][1], hist[1][1]))


def test_two_rank_entry_point(tmp_path, dev):
    """torchrun, 2 ranks (both on the one GPU of the box, gloo control plane because RCCL refuses two ranks on
    one device): samples of every batch are sharded, gradients all-reduced, rank 0 alone writes the files."""
    import subprocess
    import sys
    import pandas as pd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(tmp_path / "real_graphs"); os.makedirs(tmp_path / "multi-graph-1" / "Experiments-seed2-toy")
    G = FC.mk_graph(str(tmp_path / "real_graphs" / "toy.pkl"), 60, 180, 4)
    n = G.number_of_nodes()
    rng = np.random.default_rng(1)
    seeds = [sorted(rng.choice(n, 2, replace=False).tolist()) for _ in range(8)]
    argv = ["--lr", "0.01", "--epochs", "2", "--hidden", "64", "--I_indices"] + [str(s) for s in seeds] + \
           ["--beta"] + ["0.3"] * 8 + ["--gamma"] + ["0.2"] * 8 + \
           ["--deltaT", "0.5", "--maxTime", "6", "--sim", "100", "--trial", "0", "--dataset", "./real_graphs/toy",
            "--path_to_save", "./multi-graph-1/Experiments-seed2-toy", "--batch_size", "4",
            "--train_val_test_ratio", "0.5", "0.25", "0.25", "--model", "ode_nn"]
    env = dict(os.environ, GNODE_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(root, "gn-ode-sir_amd", "scripts", "ode_nn_ngraph_sim.py")] + argv
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    df = pd.read_csv(tmp_path / "multi-graph-1" / "Experiments-seed2-toy" / "Metrics-trials-toy")
    assert len(df) == 1 and np.isfinite(df["val_loss"][0]) and np.isfinite(df["test_loss"][0])


def test_runner_loss_matches_reference_epoch_loops(dev):
    """SURVEY 8a row A6 through the PRODUCT's code: Runner._loss_sum, train_epoch and evaluate against the numbers
    the reference's own train() / test() loops (ode_nn_ngraph_sim.py:208-296; loss expression :234, element
    weighting :248-249, :265-266, :290-294) produced on the same weights, samples and labels
    (tests/golden/make_golden_fullsize.py -> loss_epoch_karate.npz).  lr = 0 on both sides, so the weights
    stay put and the epoch mean is independent of the shuffle."""
    import torch
    import scipy.sparse as sp
    import gnode_oracle as O
    from gnode import synth
    from gnode.ode_nn_ngraph_sim import ODEBlock, ODEfunc
    from gnode.trainer import Runner
    from golden.labels import closed_form_labels
    d = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "loss_epoch_karate.npz")))
    n, H, maxTime, deltaT, NS = int(d["n"]), int(d["H"]), int(d["maxTime"]), float(d["deltaT"]), int(d["NS"])
    rp, ci = O.csr_from_edges(n, d["edges"])
    A = sp.csr_matrix((np.ones(ci.shape[0]), ci, rp), shape=(n, n))
    P = synth.linear_params(H, seed=int(d["param_seed"]))
    x = torch.from_numpy(synth.samples(n, NS, H, seed=int(d["sample_seed"])))
    y = torch.from_numpy(closed_form_labels(NS, n, maxTime))
    xs, ys = [x[i] for i in range(NS)], [y[i] for i in range(NS)]
    for use_graphs in (False, True):                      # eager loop and HIP-graph replay take different code paths
        model = ODEBlock(maxTime, deltaT, n, [0], H, ODEfunc(A, 0.2, 0.1, H, dev), dev).to(dev)
        model.load_state_dict({**model.state_dict(), **{k: torch.from_numpy(v) for k, v in P.items()}})
        run = Runner(model, 0.0, maxTime, deltaT, dev, stack=True, use_graphs=use_graphs)
        # one batch: the loss SUM over elements / element count == the reference's criterion value (:234)
        xb, yb = torch.stack(xs[:2]).to(dev), torch.cat(ys[:2], 0).to(dev)
        with torch.no_grad():
            ls = float(run._loss_sum(xb, yb)) / (2 * n * (maxTime - 1) * 3)
        assert abs(ls - float(d["test_all"][0])) <= 1e-6
        tr, _ = run.train_epoch(xs, ys, 2, epoch=0)       # batches of 2, 2, 1 in a shuffled order
        assert abs(tr - float(d["train_loss"])) <= 1e-6
        sd = model.state_dict()
        assert all(torch.equal(sd[k].cpu(), torch.from_numpy(v)) for k, v in P.items())      # lr = 0: nothing moved
        va, _ = run.evaluate(xs, ys, 3)
        assert abs(va - float(d["val_loss"])) <= 1e-6
        te, per = run.evaluate(xs, ys, 2)
        assert abs(te - float(d["test_loss"])) <= 1e-6
        assert np.max(np.abs(np.asarray(per) - d["test_all"])) <= 1e-6


@pytest.mark.parametrize("T,rows,t0,ydt", [(30, 1000, 1, "float32"), (30, 1000, 1, "float64"), (5, 7, 1, "float32"),
                                           (200, 130, 1, "float64"), (20, 34 * 5, 0, "float32"), (3, 4097, 2, "float64")])
def test_fused_l1_loss_matches_the_torch_expression(T, rows, t0, ydt, dev):
    """csrc/gnode_loss.hip against the loss expression the reference evaluates with torch ops
    (ode_nn_ngraph_sim.py:230-234: cat, transpose, [:, 1:, :], L1Loss) and torch autograd's gradient of it: value to
    float64 round-off of the summation order, gradient exactly; ragged row blocks, label rows longer than a few per
    LDS block, fp32 and fp64 labels; two runs agree bitwise."""
    import torch
    from gnode.autograd import l1_loss_sum
    gen = torch.Generator().manual_seed(T * 1000 + rows)
    S, I, R = (torch.rand(T, rows, 1, generator=gen).to(dev).requires_grad_(True) for _ in range(3))
    y = torch.rand(rows, T, 3, generator=gen, dtype=getattr(torch, ydt)).to(dev)
    with torch.no_grad():
        y[::3, :, 0] = S[:, ::3, 0].T.to(y.dtype)                     # exact ties: sign 0, as torch's abs backward
    pred = torch.cat((S, I, R), -1).transpose(0, 1)[:, t0:, :]
    want = (pred.to(y.dtype) - y[:, t0:, :]).abs().double().sum()
    gw = torch.autograd.grad(want * 0.37, (S, I, R))
    got = l1_loss_sum(S, I, R, y, t0)
    assert got.dtype == torch.float64 and abs(float(got.detach()) - float(want.detach())) <= 1e-12 * float(want.detach())
    gg = torch.autograd.grad(got * 0.37, (S, I, R))
    for a, b in zip(gg, gw):
        assert a.shape == b.shape and torch.equal(a, b.to(a.dtype))
    again = l1_loss_sum(S, I, R, y, t0)
    assert float(again.detach()) == float(got.detach())
    with torch.no_grad():                                              # evaluation: no sign tensor is produced
        assert float(l1_loss_sum(S, I, R, y, t0)) == float(got.detach())
