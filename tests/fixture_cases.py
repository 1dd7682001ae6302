"""Inputs of the gradient fixtures (tests/golden/*.npz), rebuilt from the seeds they store, and the models the GPU tests run
them through: shared by the CPU checks of the float64 restatement (oracle/gnode_restate.py) and the GPU checks of the
product, so both hold the same inputs to the same float64 numbers."""
import importlib.util
import os
import pickle

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
MULTI = ["real_multi_4-2-3-1-0-4-2-3_H8_T20", "real_multi_4-4-4-4-4-4-4-4_H8_T20"]     # compositions A and B
SINGLE = ["real_single_fbsocial_H64_T30", "real_single_wikivote_H64_T30"]
WIKI = 4                                                                             # index of wiki-vote in real_graphs.npz
VJP_CASES = ["rhs_vjp_karate_B2_H64", "rhs_vjp_loops40_B3_H8", "rhs_vjp_heavy_B1_H64", "rhs_vjp_karate_B1_H128"]

_synth_mod = None


def synth():
    """gnode/synth.py on its own (numpy only: importing the gnode package would load the HIP library)"""
    global _synth_mod
    if _synth_mod is None:
        spec = importlib.util.spec_from_file_location("_synth_real", os.path.join(os.path.dirname(HERE), "gn-ode-sir_amd", "gnode", "synth.py"))
        _synth_mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_synth_mod)
    return _synth_mod


def graphs():
    """[(rowptr, col)] of dolphins, fb-food, fb-social, openflights, wiki-vote (largest components, create_graphs' order)."""
    d = np.load(os.path.join(GOLDEN, "real_graphs.npz"))
    return [(d[f"indptr{j}"], d[f"indices{j}"]) for j in range(len(d["names"]))]


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


# --------------------------------------------------------------------------- real-graph fixtures (make_golden_realgraphs.py)
def inputs(d, gs):
    """(x, P, y) of a real-graph fixture: multi -> x [sumN, 3+H], y [sumN, T, 3]; single -> x [1, n, 3+H], y [n, T, 3]."""
    from golden.labels import closed_form_labels
    sy = synth()
    H, maxTime = int(d["H"]), int(d["maxTime"])
    P = sy.linear_params(H, seed=int(d["param_seed"]))
    if "picks" in d:
        xs = []
        for j, p in enumerate(d["picks"]):
            xi = sy.samples(gs[p][0].shape[0] - 1, 1, H, seed=int(d["sample_seed"]) + j)[0]
            xi[0, 3 + 2] = p + 1                                                   # the graph marker, ode_nn_ngraphs.py:333
            xs.append(xi)
        x = np.concatenate(xs, 0)
        x[:, 3] *= np.float32(d["beta_scale"])
    else:
        n = gs[int(d["graph"])][0].shape[0] - 1
        x = sy.samples(n, 1, H, seed=int(d["sample_seed"]))
        x[..., 3] *= np.float32(d["beta_scale"])
    rows = x.shape[0] if x.ndim == 2 else x.shape[1]
    y = closed_form_labels(1, rows, maxTime).reshape(rows, maxTime, 3)
    return x, P, y


# --------------------------------------------------------------------------- input-gradient and exact-gradient fixtures
def decode(d):
    """(x, P, y, csr, gs) of an input_grad_* / discrete_* fixture: x as the drop-in ODEBlock takes it -- [sumN, 3+H] for a
    multi-graph batch ("picks"), else [B, n, 3+H] on a real graph ("graph") or a synthetic one ("edges") --, labels y
    [rows, T, 3], csr the batch's (rowptr, col) (the concatenated CSR for a multi-graph batch), gs the real graphs (None for
    a synthetic graph)."""
    import gnode_oracle as O
    if "picks" in d or "graph" in d:
        gs = graphs()
        x, P, y = inputs(d, gs)
        csr = O.concat_csr(gs, [int(p) for p in d["picks"]])[:2] if "picks" in d else gs[int(d["graph"])]
        return x, P, y, csr, gs
    from golden.labels import closed_form_labels
    n, B, H, maxTime = int(d["n"]), int(d["B"]), int(d["H"]), int(d["maxTime"])
    x = synth().samples(n, B, H, seed=int(d["sample_seed"]))
    P = synth().linear_params(H, seed=int(d["param_seed"]))
    y = closed_form_labels(B, n, maxTime).reshape(B * n, maxTime, 3)
    return x, P, y, O.csr_from_edges(n, d["edges"]), None


def restate_args(d):
    """(x2d, P, csr, dts, L) of an input_grad_* / discrete_* fixture, the arguments of gnode_restate.adjoint / exact_grads:
    its inputs, the fp32 step sizes of its grid and the reference's L1 loss at the integer times."""
    import gnode_oracle as O
    import gnode_restate as RS
    x, P, y, csr, _ = decode(d)
    maxTime, deltaT = int(d["maxTime"]), float(d["deltaT"])
    out_rows = [int(i / deltaT) for i in range(maxTime)]
    return x.reshape(-1, x.shape[-1]), P, csr, O.step_sizes(O.time_grid(maxTime, deltaT)), RS.l1_loss_of(y, out_rows)


def adj(rp, ci):
    """the graph as the drop-in ODEfunc takes it: a scipy CSR adjacency"""
    import scipy.sparse as sp
    n = rp.shape[0] - 1
    return sp.csr_matrix((np.ones(ci.shape[0]), ci, rp), shape=(n, n))


def gpu_case(name, dev):
    """(fixture, model, x as the model takes it, labels [rows, T, 3]) of one fixture, the fixture's parameters loaded"""
    import torch
    from gnode import ode_nn_ngraph_sim as single, ode_nn_ngraphs as multi
    d = load(name)
    H, maxTime, deltaT, method = int(d["H"]), int(d["maxTime"]), float(d["deltaT"]), str(d["method"])
    x, P, y, (rp, ci), gs = decode(d)
    if "picks" in d:
        model = multi.ODEBlock(maxTime, deltaT, H, multi.ODEfunc([adj(*rc) for rc in gs], H, dev), dev)
    else:
        model = single.ODEBlock(maxTime, deltaT, rp.shape[0] - 1, [0], H, single.ODEfunc(adj(rp, ci), 0.2, 0.1, H, dev), dev,
                                method=method)
    model = model.to(dev)
    model.load_state_dict({**model.state_dict(), **{k: torch.from_numpy(v) for k, v in P.items()}})
    return d, model, torch.from_numpy(x).to(dev), y


def gpu_loss(d, model, xt, y, fused):
    """the reference's L1 loss of the model's outputs at the integer times: subsampled inside the forward (fused) or after"""
    import torch
    from gnode import ops
    from gnode.autograd import l1_loss_sum
    maxTime, deltaT = int(d["maxTime"]), float(d["deltaT"])
    rows_out = ops.subsample_rows(maxTime, deltaT)
    if fused:
        S, I, R = model(xt, out_rows=rows_out)
    else:
        S, I, R = (a[torch.from_numpy(rows_out.astype(np.int64)).to(xt.device)] for a in model(xt))
    rows = y.shape[0]
    return l1_loss_sum(S, I, R, torch.from_numpy(y).to(xt.device), 1) / (rows * (maxTime - 1) * 3)


def mk_graph(path, n, m, seed):
    """a connected G(n, m) graph pickled where the drop-in scripts look for a dataset"""
    import networkx as nx
    G = nx.gnm_random_graph(n, m, seed=seed)
    G = nx.convert_node_labels_to_integers(G.subgraph(max(nx.connected_components(G), key=len)).copy(), ordering="sorted")
    pickle.dump(G, open(path, "wb"))
    return G


# --------------------------------------------------------------------------- RHS-VJP and RK4-adjoint fixtures
def vjp_inputs(rows: int, H: int, seed: int, sample_rows: int):
    """State y [4*rows, H] (S, I, R uniform in [0, 1.5); beta, gamma per sample in columns 0, 1 of the 4th slab, the other
    columns 0) and cotangent v (standard normal), float32.  sample_rows: rows per sample (beta, gamma are per sample)."""
    rng = np.random.default_rng(seed)
    y = rng.uniform(0, 1.5, size=(4 * rows, H)).astype(np.float32)
    y[3 * rows:] = 0.0
    B = rows // sample_rows
    y[3 * rows:, 0] = np.repeat(rng.uniform(0.1, 0.5, B), sample_rows)
    y[3 * rows:, 1] = np.repeat(rng.uniform(0.1, 0.5, B), sample_rows)
    v = rng.normal(size=(4 * rows, H)).astype(np.float32)
    return y, v


def multi_inputs(ns, picks, H: int, seed: int):
    """Multi-graph state [4, sumN, H] with the sample markers (graph index + 1 at each sample's first node, column 2 of the
    4th slab, ode_nn_ngraphs.py:55), and the cotangent."""
    rng = np.random.default_rng(seed)
    tot = sum(ns[p] for p in picks)
    y = rng.uniform(0, 1.5, size=(4, tot, H)).astype(np.float32)
    y[3] = 0.0
    o = 0
    for p in picks:
        y[3, o:o + ns[p], 0] = rng.uniform(0.1, 0.5)
        y[3, o:o + ns[p], 1] = rng.uniform(0.1, 0.5)
        y[3, o, 2] = p + 1
        o += ns[p]
    v = rng.normal(size=(4, tot, H)).astype(np.float32)
    return y, v


def load_vjp_case(name):
    """(rowptr, col, y, v, P, fixture dict) of a single-graph VJP fixture (make_golden_rhs_vjp.py)."""
    import gnode_oracle as O
    d = load(name)
    n, B, H = int(d["n"]), int(d["B"]), int(d["H"])
    if "graph_seed" in d:
        rp, ci = synth().heavy_tail_csr(n, int(d["m"]), seed=int(d["graph_seed"]))
    else:
        rp, ci = O.csr_from_edges(n, d["edges"])
    y, v = vjp_inputs(B * n, H, int(d["input_seed"]), n)
    P = synth().linear_params(H, seed=int(d["param_seed"]))
    return rp, ci, y, v, P, d


def load_multi_case(name="rhs_vjp_multi_0-2-1_H8"):
    """(graphs [(rowptr, col)], picks, y [4, sumN, H], v, P, fixture dict)."""
    import gnode_oracle as O
    d = load(name)
    H = int(d["H"])
    gs = [O.csr_from_edges(int(d[f"n{j}"]), d[f"edges{j}"]) for j in range(3)]
    ns = [int(d[f"n{j}"]) for j in range(3)]
    picks = [int(p) for p in d["picks"]]
    y, v = multi_inputs(ns, picks, H, int(d["input_seed"]))
    return gs, picks, y, v, synth().linear_params(H, seed=int(d["param_seed"])), d


def rk4_case(name):
    """(rowptr, col, x [B, n, 3+H], P, labels [rows, T, 3], fixture dict) of an RK4-adjoint fixture (make_golden_rk4_adjoint.py)."""
    import gnode_oracle as O
    from golden.labels import closed_form_labels
    d = load(name)
    n, B, H, maxTime = int(d["n"]), int(d["B"]), int(d["H"]), int(d["maxTime"])
    rp, ci = O.csr_from_edges(n, d["edges"])
    x = synth().samples(n, B, H, seed=int(d["sample_seed"]))
    P = synth().linear_params(H, seed=int(d["param_seed"]))
    y = closed_form_labels(B, n, maxTime).reshape(B * n, maxTime, 3)
    return rp, ci, x, P, y, d
