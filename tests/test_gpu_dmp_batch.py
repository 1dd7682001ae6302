"""GPU: the DMP baseline for a batch of samples in one call (gnode_dmp_batch_f32 through gnode.dmp.dmp_batch and through the
C entry), on the cases of tests/baseline_cases.py from the states of sir_model.mixed_init.  A sample inside a batch is held
to its solo run (DMP_SIR.run -> gnode_dmp_init_f32) BIT FOR BIT, in both forms of the kernel and at the sizes where the
library changes form; the sizes come from gnode_dmp_batch_lds_bytes, not from a formula restated here."""
import functools
import os
import pickle

import numpy as np
import pytest

from baseline_cases import DMP_CASES, RTOL, dmp_parent, er as _er, gammas as _gammas, is_parents, rel as _rel, weights as _weights
from sir_cases import dev, state as _state  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = ["hub", "isolated", "T2", "T3", "nnz0", "w_zero", "gamma_01", "w_one"]
CASE_SEED = {name: 700 + 10 * i for i, name in enumerate(CASES)}
SCALE = [1.0, 0.5, 0.8125]
LDS_WORKGROUP = 160 * 1024          # what a gfx950 workgroup may declare
T_FORMS = 6
FORM_TAGS = ["small", "mid", "last_fit", "first_unfit"]
FORM_SCALE = [1.0, 0.75]


def _matrix(rp, ci, w):
    import scipy.sparse as sp
    n = len(rp) - 1
    return sp.csr_matrix((np.asarray(w, dtype=np.float64), ci, rp), shape=(n, n))


def _w(rp, ci, seed):
    """Weights that are not symmetric in value, sized to the mean degree so that long rows neither die out nor saturate."""
    s = min(1.0, 5.0 * (len(rp) - 1) / max(len(ci), 1))
    return _weights(len(ci), 0.05 * s, 0.4 * s, seed)


def _states(n, seed, B):
    from sir_model import mixed_init
    return [mixed_init(n, seed + b)[0] for b in range(B)]


@functools.lru_cache(maxsize=None)
def batch_case(name):
    """(case, matrix, B = 3 mixed states, gamma [3, n]) of a DMP case, read-only; nothing here touches the GPU."""
    c = DMP_CASES[name]()
    n = len(c["rp"]) - 1
    ps = _states(n, CASE_SEED[name], 3)
    gam = np.stack([c["gam"], (c["gam"] * np.float32(0.5)).astype(np.float32), _gammas(n, CASE_SEED[name] + 5)])
    for a in ps + [gam]:
        a.setflags(write=False)
    return c, _matrix(c["rp"], c["ci"], c["w"]), ps, gam


@functools.lru_cache(maxsize=None)
def batch_out(name):
    """The batch of `batch_case(name)` through dmp_batch, once: a float32 host tensor [3, T, n, 3] that nobody writes to."""
    from gnode.dmp import dmp_batch
    c, M, ps, gam = batch_case(name)
    return dmp_batch(M, [_state(p) for p in ps], gam, c["T"], scale=SCALE).cpu()


def _solo(M, gamma, start, T):
    from gnode.dmp import DMP_SIR
    return DMP_SIR(M, gamma).run(start, T)


def _lds_bytes(rp, ci):
    from gnode import _lib
    from gnode.graph import DeviceGraph
    g = DeviceGraph(rp, ci)
    return int(_lib.load().gnode_dmp_batch_lds_bytes(g.handle))


# ------------------------------------------------------------------ bit equality with the solo run
@pytest.mark.parametrize("name", CASES)
def test_batch_sample_is_its_solo_run(name, dev):
    import torch
    c, M, ps, gam = batch_case(name)
    got = batch_out(name)
    assert got.shape == (3, c["T"], M.shape[0], 3) and got.dtype == torch.float32
    for b in range(3):
        want = _solo(M * SCALE[b], gam[b], _state(ps[b]), c["T"]).cpu()
        assert torch.isfinite(want).all()
        assert torch.equal(got[b], want), f"{name}: sample {b}"


def test_one_sample_with_shared_weights_is_dmp_sir_run(dev):
    import torch
    from gnode.dmp import dmp_batch
    for name in ("T3", "hub"):
        c, M, ps, gam = batch_case(name)
        got = dmp_batch(M, [_state(ps[0])], gam[0], c["T"])
        assert got.shape == (1, c["T"], M.shape[0], 3)
        assert torch.equal(got[0], _solo(M, gam[0], _state(ps[0]), c["T"])), name


def test_seed_lists_are_the_seed_list_runs(dev):
    import torch
    from gnode.dmp import dmp_batch
    for name in ("w_zero", "isolated", "hub"):
        c, M, _, gam = batch_case(name)
        n = M.shape[0]
        starts = [c["seeds"], [n - 1], []]
        got = dmp_batch(M, starts, gam[1], c["T"])
        for b, seeds in enumerate(starts):
            assert torch.equal(got[b], _solo(M, gam[1], seeds, c["T"])), f"{name}: sample {b}"


# ------------------------------------------------------------------ the model's bars
@pytest.mark.parametrize("name", ["hub", "w_zero"])
def test_batch_meets_the_models_bars(name, dev):
    from sir_init_model import dmp_sir_init
    c, M, ps, gam = batch_case(name)
    out = batch_out(name).numpy()
    for b in range(3):
        w = (M.data * SCALE[b]).astype(np.float32)
        o32, o64 = (dmp_sir_init(c["rp"], c["ci"], w, gam[b], ps[b], c["T"], d) for d in ("float32", "float64"))
        yard, gpu_err = _rel(o32, o64), _rel(out[b], o64)
        print(f"dmp batch {name}[{b}]: gpu_err={gpu_err:.3e} yard={yard:.3e} vs_fp32_restatement={_rel(out[b], o32):.3e}")
        assert _rel(out[b], o32) <= RTOL
        assert gpu_err <= max(4 * yard, 1e-6)
        assert np.max(np.abs(out[b].astype(np.float64).sum(-1) - 1.0)) <= 1e-5
        assert np.array_equal(out[b][0], ps[b].astype(np.float32))             # row 0 is the state itself


# ------------------------------------------------------------------ both forms and their boundaries
N_FORMS = 120


@functools.lru_cache(maxsize=None)
def form_graphs():
    """{tag: (rp, ci, lds bytes)} at n = 120: a graph whose one-workgroup form needs <= 64 KiB, one between 64 KiB and the
    workgroup's 160 KiB, the largest m that still fits, and the next m, which does not.  The sizes are the library's answers."""
    def at(m):
        rp, ci, _ = _er(N_FORMS, m, 40)
        return rp, ci, _lds_bytes(rp, ci)
    lo, hi = 2500, N_FORMS * (N_FORMS - 1) // 2                     # lo fits, hi does not
    assert at(lo)[2] <= LDS_WORKGROUP < at(hi)[2]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if at(mid)[2] <= LDS_WORKGROUP else (lo, mid)
    g = {"small": at(300), "mid": at(2500), "last_fit": at(lo), "first_unfit": at(hi)}
    assert g["small"][2] <= 64 * 1024 < g["mid"][2] <= LDS_WORKGROUP
    assert g["last_fit"][2] <= LDS_WORKGROUP < g["first_unfit"][2]
    return g


def _form_inputs(tag, B, seed):
    rp, ci, _ = form_graphs()[tag]
    M = _matrix(rp, ci, _w(rp, ci, seed))
    return M, _states(N_FORMS, seed + 1, B), np.stack([_gammas(N_FORMS, seed + 10 + b) for b in range(B)])


def form_out(tag):
    """(inputs, the batch of two samples on a form graph through dmp_batch)"""
    from gnode.dmp import dmp_batch
    M, ps, gam = _form_inputs(tag, 2, 50)
    return (M, ps, gam), dmp_batch(M, [_state(p) for p in ps], gam, T_FORMS, scale=FORM_SCALE)


def form_solo(inputs, b):
    M, ps, gam = inputs
    return _solo(M * FORM_SCALE[b], gam[b], _state(ps[b]), T_FORMS)


@pytest.mark.parametrize("tag", FORM_TAGS)
def test_each_form_and_boundary_is_the_solo_run(tag, dev):
    import torch
    inputs, got = form_out(tag)
    for b in range(2):
        want = form_solo(inputs, b)
        assert torch.isfinite(want).all() and float((want[0, :, 0] - want[-1, :, 0]).max()) > 0.05       # something spread
        assert torch.equal(got[b], want), f"{tag}: sample {b}"


# ------------------------------------------------------------------ the parent's bits
def _batch_need(M, B):
    from gnode import _lib
    from gnode.dmp import DmpGraph
    G = DmpGraph(M)                                                 # (kept: the handle dies with it)
    return int(_lib.load().gnode_dmp_batch_workspace_bytes(G.graph.handle, B))


@pytest.mark.parametrize("name", CASES)
def test_batch_and_solo_runs_are_the_parents_bits(name, dev):
    """tests/golden/dmp_parent.json: what the library of commit 893d874 returned on an MI355X, when the solo entries had kernels
    of their own.  Equality of digests; since then a solo call is the general form with one sample, so for the graphs that
    the general form serves this, not the comparison with the solo run, is what holds the arithmetic."""
    c, M, ps, gam = batch_case(name)
    assert is_parents(f"dmp_batch/{name}", batch_out(name))
    assert _batch_need(M, 3) == dmp_parent()[f"dmp_batch/{name}"]["batch_workspace_bytes"]
    for b in range(3):
        assert is_parents(f"dmp_init_f32/{name}/{b}", _solo(M * SCALE[b], gam[b], _state(ps[b]), c["T"])), f"sample {b}"


@pytest.mark.parametrize("tag", FORM_TAGS)
def test_each_form_and_boundary_is_the_parents_bits(tag, dev):
    inputs, got = form_out(tag)
    assert is_parents(f"dmp_batch/form/{tag}", got)
    assert _batch_need(inputs[0], 2) == dmp_parent()[f"dmp_batch/form/{tag}"]["batch_workspace_bytes"]
    for b in range(2):
        assert is_parents(f"dmp_init_f32/form/{tag}/{b}", form_solo(inputs, b)), f"sample {b}"


def test_which_form_serves_which_case(dev):
    """hub is the general form with a long serial row; isolated and nnz0 are the one-workgroup form with empty rows / no edges."""
    sizes = {name: _lds_bytes(DMP_CASES[name]()["rp"], DMP_CASES[name]()["ci"]) for name in ("hub", "isolated", "nnz0")}
    assert sizes["hub"] > LDS_WORKGROUP
    assert 0 < sizes["isolated"] <= LDS_WORKGROUP and 0 < sizes["nnz0"] <= LDS_WORKGROUP
    assert np.diff(DMP_CASES["hub"]()["rp"]).max() > 256 and np.diff(DMP_CASES["isolated"]()["rp"]).min() == 0


def test_more_samples_than_one_chunk_of_the_trainer(dev):
    import torch
    from gnode.dmp import DmpGraph, dmp_batch
    c, M, _, _ = batch_case("w_zero")
    n, B = M.shape[0], 70
    ps = _states(n, 900, B)
    rng = np.random.default_rng(31)
    scale, gam = rng.uniform(0.3, 1.0, B), rng.uniform(0.1, 0.5, B)
    got = dmp_batch(DmpGraph(M), [_state(p) for p in ps], gam, c["T"], scale=scale)      # B numbers: one gamma per sample
    assert got.shape[0] == B
    for b in range(B):
        assert torch.equal(got[b], _solo(M * scale[b], [gam[b]] * n, _state(ps[b]), c["T"])), f"sample {b}"


# ------------------------------------------------------------------ the C entry
class Entry:
    """gnode_dmp_batch_f32 on one graph with device tensors of the caller's making."""

    def __init__(self, rp, ci, dev):
        from gnode import _lib
        from gnode.graph import DeviceGraph
        self.lib, self.dev, self.g = _lib.load(), dev, DeviceGraph(rp, ci)

    def need(self, B):
        return int(self.lib.gnode_dmp_batch_workspace_bytes(self.g.handle, B))

    def up(self, a, dtype=np.float32):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.dev)

    def call(self, w, w_stride, gam, gamma_stride, init, B, T, out, ws, nbytes=None):
        from gnode import _lib
        return self.lib.gnode_dmp_batch_f32(self.g.handle, _lib.ptr(w), w_stride, _lib.ptr(gam), gamma_stride, _lib.ptr(init), B, T,
                                            _lib.ptr(out), _lib.ptr(ws), ws.numel() if nbytes is None else nbytes, _lib.stream_ptr())


def _entry_graphs():
    c = DMP_CASES["T3"]()
    return {"one_workgroup": (c["rp"], c["ci"]), "general": form_graphs()["first_unfit"][:2]}


@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_shared_and_per_sample_strides(form, dev):
    import torch
    rp, ci = _entry_graphs()[form]
    n, nnz, B, T = len(rp) - 1, len(ci), 3, 5
    e = Entry(rp, ci, dev)
    assert (e.lib.gnode_dmp_batch_lds_bytes(e.g.handle) <= LDS_WORKGROUP) == (form == "one_workgroup")
    ps = _states(n, 60, B)
    W = np.stack([_w(rp, ci, 61 + b) for b in range(B)])
    G = np.stack([_gammas(n, 65 + b) for b in range(B)])
    init, ws = e.up(np.stack(ps)), torch.empty(e.need(B), dtype=torch.uint8, device=dev)
    for w_shared in (True, False):                                  # (w_stride, gamma_stride) = (0, n) and (nnz, 0)
        w, gam = (W[0], G) if w_shared else (W, G[0])
        out = torch.zeros((B, T, n, 3), dtype=torch.float32, device=dev)
        assert e.call(e.up(w), 0 if w_shared else nnz, e.up(gam), n if w_shared else 0, init, B, T, out, ws) == 0, \
            e.lib.gnode_last_error().decode()
        for b in range(B):
            want = _solo(_matrix(rp, ci, W[0 if w_shared else b]), G[b if w_shared else 0], _state(ps[b]), T)
            assert torch.equal(out[b], want), f"{form}, shared weights {w_shared}: sample {b}"


@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_no_state_is_carried_over_in_the_workspace(form, dev):
    import torch
    rp, ci = _entry_graphs()[form]
    n, nnz, B, T = len(rp) - 1, len(ci), 2, 6
    e = Entry(rp, ci, dev)
    ws = torch.full((e.need(B),), 0xFF, dtype=torch.uint8, device=dev)          # NaNs, should anything read before it writes
    outs = []
    for seed in (70, 80, 70):
        w = e.up(np.stack([_w(rp, ci, seed + b) for b in range(B)]))
        gam = e.up(np.stack([_gammas(n, seed + 3 + b) for b in range(B)]))
        out = torch.zeros((B, T, n, 3), dtype=torch.float32, device=dev)
        assert e.call(w, nnz, gam, n, e.up(np.stack(_states(n, seed + 6, B))), B, T, out, ws) == 0, e.lib.gnode_last_error().decode()
        outs.append(out)
    assert torch.isfinite(outs[0]).all() and not torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_refusals_leave_out_untouched_and_a_good_call_is_served(form, dev):
    import torch
    from gnode import _lib
    ARG, WORKSPACE = -1, -3                                         # GNODE_ERR_ARG, GNODE_ERR_WORKSPACE of include/gnode.h
    rp, ci = _entry_graphs()[form]
    n, nnz, B, T = len(rp) - 1, len(ci), 2, 4
    e = Entry(rp, ci, dev)
    ps = _states(n, 90, B)
    W, G = _w(rp, ci, 91), _gammas(n, 92)
    w, gam, init = e.up(W), e.up(G), e.up(np.stack(ps))
    need = e.need(B)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.full((B, T, n, 3), -7.0, dtype=torch.float32, device=dev)
    assert e.call(w, 0, gam, 0, init, B, T, out, ws, need - 1) == WORKSPACE
    assert e.call(w, 0, gam, 0, init, 0, T, out, ws) == ARG
    assert e.call(w, 0, gam, 0, init, B, 1, out, ws) == ARG
    for ws_, gs_ in ((1, 0), (nnz - 1, 0), (0, 1), (0, n + 1), (n, 0), (-nnz, 0)):
        assert e.call(w, ws_, gam, gs_, init, B, T, out, ws) == ARG, (ws_, gs_)
    for missing in ("w", "gam", "init", "out", "ws"):
        a = dict(w=w, gam=gam, init=init, out=out, ws=ws)
        a[missing] = None
        assert e.lib.gnode_dmp_batch_f32(e.g.handle, _lib.ptr(a["w"]), 0, _lib.ptr(a["gam"]), 0, _lib.ptr(a["init"]), B, T,
                                         _lib.ptr(a["out"]), _lib.ptr(a["ws"]), need, _lib.stream_ptr()) == ARG, missing
    k = nnz // 2                                                    # one directed entry out of the middle of the CSR
    row = int(np.searchsorted(rp, k, side="right") - 1)
    rp2 = rp.copy(); rp2[row + 1:] -= 1
    e2 = Entry(rp2, np.delete(ci, k), dev)
    ws2 = torch.empty(e2.need(B), dtype=torch.uint8, device=dev)
    assert e2.call(e.up(np.delete(W, k)), 0, gam, 0, init, B, T, out, ws2) == ARG
    assert "symmetric" in e2.lib.gnode_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert e.call(w, 0, gam, 0, init, B, T, out, ws) == 0, e.lib.gnode_last_error().decode()
    for b in range(B):
        assert torch.equal(out[b], _solo(_matrix(rp, ci, W), G, _state(ps[b]), T))


# ------------------------------------------------------------------ the drop-in script
def test_main_dmp_prints_each_samples_solo_loss(tmp_path, monkeypatch, dev):
    import contextlib
    import io
    import fixture_cases as FC
    from gnode.dmp import DMP_SIR
    from gnode.ode_nn import create_graph
    from gnode.trainer import _decode_seeds, _labels_of, main_dmp, parser_single, split_indices
    monkeypatch.chdir(tmp_path)
    os.makedirs("real_graphs"); os.makedirs("multi-graph-1/Experiments-seed2-toy")
    G = FC.mk_graph("real_graphs/toy.pkl", 80, 240, 1)
    n = G.number_of_nodes()
    rng = np.random.default_rng(0)
    S = 10
    seeds = [sorted(rng.choice(n, 2, replace=False).tolist()) for _ in range(S)]
    argv = ["--I_indices"] + [str(s) for s in seeds] + ["--beta"] + [f"{b:.3f}" for b in rng.uniform(0.1, 0.5, S)] + \
           ["--gamma"] + [f"{g:.3f}" for g in rng.uniform(0.1, 0.5, S)] + \
           ["--maxTime", "8", "--sim", "200", "--dataset", "./real_graphs/toy", "--path_to_save", "./multi-graph-1/Experiments-seed2-toy",
            "--train_val_test_ratio", "0.2", "0.1", "0.7", "--model", "dmp"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert main_dmp(argv) == 0
    lines = buf.getvalue().splitlines()
    assert lines[0] == str(n) and lines[-2].startswith("DMP baseline Loss: ") and lines[-1].startswith("Time inference baseline: ")
    body = lines[1:-2]
    args = parser_single().parse_args(argv)
    _decode_seeds(args)
    assert pickle.load(open(args.path_to_save + "/initial-seed.pkl", "rb")) == seeds
    G2, A, _ = create_graph(50, args.dataset)
    ys = [np.stack([np.asarray(a) for a in lab], -1) for lab in _labels_of(args, G2)]      # the label files main_dmp wrote
    te = split_indices(S, args.train_val_test_ratio)[2]
    assert len(te) == 7 and body[0::2] == ["dmp"] * len(te) and len(body) == 2 * len(te)    # one loss per test sample
    import scipy.sparse as sp
    A1 = sp.csr_matrix(A).astype(np.float64)
    A1.data[:] = 1.0
    loss_all, items = 0.0, 0
    for line, i in zip(body[1::2], te):
        solo = DMP_SIR(A1 * args.beta[i], [args.gamma[i]] * n).run(args.I_indices[i], args.maxTime).cpu().numpy()
        loss = float(np.abs(solo[1:].astype(np.float64) - ys[i][1:]).mean())
        assert float(line) == loss and 0 < loss < 0.5, f"sample {i}"
        loss_all += loss * 3 * n * (args.maxTime - 1)
        items += 3 * n * (args.maxTime - 1)
    assert lines[-2] == "DMP baseline Loss: {:.5f}".format(loss_all / items)
