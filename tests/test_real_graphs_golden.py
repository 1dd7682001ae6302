"""The oracle against float64 vectors the REFERENCE classes produced on the real training graphs (tests/golden/real_*.npz,
tests/golden/make_golden_realgraphs.py): configs[4]'s H = 8 multi-graph batches over 39 intervals and configs[1] / [2]'s
H = 64 single-graph runs over 59, on real topology (hub rows up to 1 065 edges, fb-food's self-loops).  Then sensitivity:
the oracle run with one known fault must miss the fixture by more than the tolerance test_gpu_real_graphs.py holds the
GPU to, so those tolerances are shown to catch a lost hub segment, a wrong batch composition or a lost interval."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import gnode_oracle as O
import fixture_cases as FC

GPU_OUT, GPU_LOSS, GPU_GRAD = 2e-5, 1e-6, 2e-4          # test_gpu_real_graphs.py's tolerances


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-12)


@functools.lru_cache(maxsize=None)
def _graphs():
    return FC.graphs()


def _forward64(d, x, gs):
    """float64 oracle forward -> pred [maxTime, rows, 3] at the rows the loss sees (get_sir_t_nodes)"""
    maxTime, deltaT = int(d["maxTime"]), float(d["deltaT"])
    P = {k: v.astype(np.float64) for k, v in FC.inputs(d, _graphs())[1].items()}
    with O.precision(np.float64):
        if x.ndim == 2:
            out = O.odeblock_forward_multi(x.astype(np.float64), P, gs, maxTime, deltaT)
        else:
            rp, ci = gs[int(d["graph"])]
            out = O.odeblock_forward_single(x.astype(np.float64), P, rp, ci, maxTime, deltaT)
    return np.stack([O.get_sir_t_nodes(a[..., 0], maxTime, deltaT) for a in out], -1)


def _loss_and_cotangent(pred, y):
    diff = pred - y.transpose(1, 0, 2)
    diff[0] = 0.0                                                                 # t = 0 excluded (ode_nn_ngraphs.py:219)
    N = diff.size - diff[0].size
    return np.abs(diff).sum() / N, np.sign(diff) / N


def _adjoint64(d, x, pred, y, gs, stop_at=1):
    maxTime, deltaT = int(d["maxTime"]), float(d["deltaT"])
    _, g = _loss_and_cotangent(pred, y)
    P = FC.inputs(d, _graphs())[1]
    rows = np.asarray([int(i / deltaT) for i in range(maxTime)])
    if x.ndim == 2:
        return O.adjoint_grads_multi(x, P, gs, maxTime, deltaT, g[..., 0], g[..., 1], g[..., 2], out_rows=rows, dtype="float64",
                                     stop_at=stop_at)
    rp, ci = gs[int(d["graph"])]
    return O.adjoint_grads_torch(x, P, rp, ci, maxTime, deltaT, g[..., 0], g[..., 1], g[..., 2], out_rows=rows, dtype="float64",
                                 stop_at=stop_at)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(fixture, x, y, pred, grads) of the oracle's float64 run on a fixture's inputs"""
    d = FC.load(name)
    x, _, y = FC.inputs(d, _graphs())
    pred = _forward64(d, x, _graphs())
    return d, x, y, pred, _adjoint64(d, x, pred, y, _graphs())


def _out_err(d, pred):
    """max over S, I, R of the distance at the kept rows, relative to each tensor's max"""
    return max(_rel(pred[d["rows_kept"], :, j], d[c]) for j, c in enumerate("SIR"))


def _grad_err(d, got):
    return max(_rel(got[k], d["G:" + k]) for k in got if k != "linearS2.bias")


def test_real_graphs_are_create_graphs_output():
    """The stored topology: symmetric, sorted, one diagonal entry per self-loop, and the node / nnz / degree figures the
    real datasets have (largest components)."""
    want = {0: (62, 318, 12, 0), 1: (620, 4193, 133, 11), 2: (1893, 27670, 255, 0), 3: (2905, 31290, 242, 0), 4: (7066, 201472, 1065, 0)}
    for j, (rp, ci) in enumerate(_graphs()):
        n = rp.shape[0] - 1
        A = sp.csr_matrix((np.ones(ci.shape[0]), ci, rp), shape=(n, n))
        assert (A != A.T).nnz == 0 and A.has_sorted_indices and A.max() == 1
        assert (n, A.nnz, int(np.diff(rp).max()), int(A.diagonal().sum())) == want[j]


@pytest.mark.parametrize("name", FC.MULTI + FC.SINGLE)
def test_oracle_matches_reference_on_real_graphs(name):
    """float64 oracle forward: the reference's float64 outputs at the kept rows to 1e-12 beyond their float32 rounding
    (half an ulp, 2^-25 on values below 1), its loss to 1e-9; the oracle's adjoint: the reference's gradients to 1e-9 relative."""
    d, x, y, pred, got = _oracle(name)
    for j, c in enumerate("SIR"):
        assert np.abs(pred[d["rows_kept"], :, j] - d[c]).max() <= 2.0 ** -25 + 1e-12, c
    loss, _ = _loss_and_cotangent(pred, y)
    assert abs(loss - float(d["loss"])) <= 1e-9
    for k, v in got.items():
        want = d["G:" + k]
        assert np.max(np.abs(v - want)) <= 1e-9 * (np.max(np.abs(want)) + 1e-12) + 1e-15, k
    # the reference's own fp32 run of the same rule is the yardstick: it must leave the GPU tolerances room
    assert _grad_err(d, {k[4:]: d[k] for k in d if k.startswith("G32:")}) <= GPU_GRAD / 4
    assert float(d["out32_err"]) <= GPU_OUT / 4


def test_concatenated_csr_is_the_references_block_diag():
    """ode_nn_ngraphs.py:65-71 rebuilds scipy.sparse.block_diag of the picked graphs on every RHS call; the concatenated
    CSR (oracle concat_csr, the product's graph.concat_csr) is that matrix, for both compositions."""
    gs = _graphs()
    for name in FC.MULTI:
        picks = [int(p) for p in FC.load(name)["picks"]]
        rp, ci, off = O.concat_csr(gs, picks)
        mats = [sp.csr_matrix((np.ones(c.shape[0]), c, r), shape=(r.shape[0] - 1,) * 2) for r, c in gs]
        bd = sp.block_diag([mats[p] for p in picks]).tocsr()
        bd.sort_indices()
        assert np.array_equal(bd.indptr, rp) and np.array_equal(bd.indices, ci)
        assert off[-1] == bd.shape[0]


def test_multi_adjoint_equals_batched_single_graph():
    """Composition B (eight wiki-vote samples): the multi-graph adjoint over the concatenated CSR with B = 1 is the
    single-graph adjoint over B = 8 copies of the graph (the block-diagonal replication of ode_nn_ngraph_sim.py)."""
    gs = _graphs()
    d, x, y, pred, want = _oracle(FC.MULTI[1])
    _, P, _ = FC.inputs(d, gs)
    maxTime, deltaT = int(d["maxTime"]), float(d["deltaT"])
    n = gs[FC.WIKI][0].shape[0] - 1
    _, g = _loss_and_cotangent(pred, y)
    rows = np.asarray([int(i / deltaT) for i in range(maxTime)])
    got = O.adjoint_grads_torch(x.reshape(8, n, x.shape[1]), P, *gs[FC.WIKI], maxTime, deltaT, g[..., 0], g[..., 1], g[..., 2],
                                out_rows=rows, dtype="float64")
    for k in want:
        assert np.max(np.abs(got[k] - want[k])) <= 1e-12 * (np.max(np.abs(want[k])) + 1e-12), k


# ---- sensitivity: each fault must move the oracle outside the GPU tolerance
def test_dropped_hub_segment_is_caught():
    """wiki-vote's 1 065-edge row loses its last 32-edge segment (the kernels cut hub rows into segments of <= 32 edges,
    in order: csrc/gnode_graph_plan.cpp) -- what a lost segment in k_hub_seg or a persistent kernel's hub path would do.
    The kept outputs catch it by orders of magnitude; the summed parameter gradients alone move by about half their
    tolerance (one row of 7 066), so the outputs are the check that holds this fault."""
    gs = _graphs()
    name = FC.SINGLE[1]
    d, x, y, _, _ = _oracle(name)
    rp, ci = gs[FC.WIKI]
    deg = np.diff(rp)
    hub = int(np.argmax(deg))
    assert deg[hub] == 1065
    lo = int(rp[hub]) + ((int(deg[hub]) - 1) // 32) * 32 - 32                     # the last full segment of the row
    keep = np.ones(ci.shape[0], dtype=bool)
    keep[lo:lo + 32] = False
    rp2 = rp.copy()
    rp2[hub + 1:] -= 32
    bad = list(gs)
    bad[FC.WIKI] = (rp2, ci[keep])
    pred = _forward64(d, x, bad)
    out_err = _out_err(d, pred)
    grad_err = _grad_err(d, _adjoint64(d, x, pred, y, bad))
    print(f"dropped hub segment: outputs off by {out_err:.1e} (tolerance {GPU_OUT:.0e}), gradients {grad_err:.1e} ({GPU_GRAD:.0e})")
    assert out_err > 10 * GPU_OUT and grad_err > GPU_GRAD / 10


def test_swapped_composition_is_caught():
    """Composition A's first two picks (wiki-vote, fb-social) swapped: the concatenated CSR still has the batch's row count,
    but the gather runs over the wrong graphs' blocks -- what a cached graph of the wrong composition would do."""
    gs = _graphs()
    d, x, y, _, _ = _oracle(FC.MULTI[0])
    picks = [int(p) for p in d["picks"]]
    assert picks[0] != picks[1]
    picks[0], picks[1] = picks[1], picks[0]
    rp, ci, off = O.concat_csr(gs, picks)
    assert off[-1] == x.shape[0]
    P = {k: v.astype(np.float64) for k, v in FC.inputs(d, gs)[1].items()}
    maxTime, deltaT = int(d["maxTime"]), float(d["deltaT"])
    with O.precision(np.float64):
        out = O.odeblock_forward_single(x[None].astype(np.float64), P, rp, ci, maxTime, deltaT)
    pred = np.stack([O.get_sir_t_nodes(a[..., 0], maxTime, deltaT) for a in out], -1)
    out_err = _out_err(d, pred)
    print(f"swapped composition: outputs off by {out_err:.1e} (tolerance {GPU_OUT:.0e})")
    assert out_err > GPU_OUT


@pytest.mark.parametrize("name", [FC.MULTI[0], FC.SINGLE[0]])
def test_missing_interval_is_caught(name):
    """The adjoint sweep stops one interval early (interval 1 -> 0 is never taken): gradients miss by more than 2e-4."""
    d, x, y, pred, _ = _oracle(name)
    err = _grad_err(d, _adjoint64(d, x, pred, y, _graphs(), stop_at=2))
    print(f"{name} missing interval: gradients off by {err:.1e} (tolerance {GPU_GRAD:.0e})")
    assert err > GPU_GRAD
