"""GPU: the DMP and mean-field baselines from an initial-state distribution (gnode_dmp_init_f32, gnode_meanfield_init_f64
through DMP_SIR.run / runge_kutta_order4 with an InitialState), at the graphs and bars of tests/test_gpu_baselines.py against
the references of tests/sir_init_model.py on the cases of tests/baseline_cases.py, and the Monte-Carlo's marginals against
DMP's on a tree, where those are exact."""
import functools

import numpy as np
import pytest

from baseline_cases import DMP_CASES, MF_ATOL, RTOL, dmp_model as _dmp_model, er as _er, rel as _rel
from sir_cases import dev, state as _state, tree_case, u32 as _u32  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = ["hub", "isolated", "T2", "T3", "nnz0", "seeds_none", "w_one", "w_zero", "gamma_01"]
INIT_SEED = {name: 401 + i for i, name in enumerate(CASES)}


@functools.lru_cache(maxsize=None)
def init_refs(name):
    """(case, p, float32 restatement, float64 yardstick, yard), computed once; nothing here touches the GPU."""
    from sir_init_model import dmp_sir_init
    from sir_model import mixed_init
    c = DMP_CASES[name]()
    p, _ = mixed_init(len(c["rp"]) - 1, INIT_SEED[name])
    with np.errstate(all="ignore"):     # w = 1: the float32 recurrence divides 0 by 0 in its last edge pass (test_gpu_baselines.py)
        o32, o64 = (dmp_sir_init(c["rp"], c["ci"], c["w"], c["gam"], p, c["T"], d) for d in ("float32", "float64"))
    for a in (p, o32, o64):
        a.setflags(write=False)
    return c, p, o32, o64, _rel(o32, o64)


def _check_bars(tag, out, o32, o64, yard):
    assert out.shape == o32.shape and out.dtype == np.float32
    gpu_err = _rel(out, o64)
    print(f"dmp init {tag}: gpu_err={gpu_err:.3e} yard={yard:.3e} vs_fp32_restatement={_rel(out, o32):.3e}")
    assert _rel(out, o32) <= RTOL
    assert gpu_err <= max(4 * yard, 1e-6)
    assert np.max(np.abs(out.astype(np.float64).sum(-1) - 1.0)) <= 1e-5


@pytest.mark.parametrize("name", CASES)
def test_dmp_mixed_state(name, dev):
    c, p, o32, o64, yard = init_refs(name)
    out = _dmp_model(c).run(_state(p), c["T"]).cpu().numpy()
    _check_bars(name, out, o32, o64, yard)
    assert np.array_equal(out[0], p.astype(np.float32))                       # row 0 is the state itself
    assert (p[:, 2] > 0).any() and out[-1, :, 2].min() >= 0


@pytest.mark.parametrize("name", ["hub", "isolated", "nnz0", "gamma_01", "w_zero"])
def test_dmp_one_hot_state_is_the_seed_list_run(name, dev):
    import torch
    from gnode.ode_nn import InitialState
    c = DMP_CASES[name]()
    m = _dmp_model(c)
    want = m.run(c["seeds"], c["T"]).clone()
    got = m.run(InitialState.from_sets(m.N, c["seeds"]), c["T"])
    assert torch.equal(got, want)
    assert torch.equal(m.run(c["seeds"], c["T"]), want)                       # ... and the seed-list path afterwards


def test_dmp_refuses_a_short_workspace_and_serves_afterwards(dev):
    import torch
    from gnode import _lib
    lib = _lib.load()
    c, p, o32, _, _ = init_refs("T3")
    m = _dmp_model(c)
    need = lib.gnode_dmp_init_workspace_bytes(m.graph.handle)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.zeros((c["T"], m.N, 3), dtype=torch.float32, device=dev)
    init = torch.from_numpy(p.astype(np.float32)).to(dev)
    call = lambda init_t, nbytes: lib.gnode_dmp_init_f32(m.graph.handle, _lib.ptr(m.weights), _lib.ptr(m.nodes_gamma), _lib.ptr(init_t),
                                                         c["T"], _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_ptr())
    assert call(init, need - 1) != 0 and call(None, need) != 0
    torch.cuda.synchronize()
    assert not out.any()
    assert call(init, need) == 0, lib.gnode_last_error().decode()
    assert _rel(out.cpu().numpy(), o32) <= RTOL


def test_counts_agree_with_dmp_on_a_tree(dev):
    """The tree case from the mixed state: 20 000 trajectories of the GPU Monte-Carlo lie within the project's per-cell 5
    sigma bound of float64 DMP, |count / sims - P| <= 5 (sqrt(P (1 - P) / sims) + 1 / sims), row 0 INCLUDED (the CPU model,
    whose counts the GPU's equal, gives a largest ratio of 3.93: a failure is a wrong rule, not noise), and gnode_dmp_init_f32
    meets the float32 bars on the same inputs."""
    import scipy.sparse as sp
    from gnode.dmp import DMP_SIR
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import edge_rates, sir_counts
    from sir_init_model import dmp_sir_init, sigma_ratio, tree_init
    n, rp, ci, w, gamma = tree_case()
    p, sims, T = tree_init(), 20000, 12
    P = dmp_sir_init(rp, ci, w, gamma, p, T, "float64")
    g = DeviceGraph(rp, ci)
    M = sp.csr_matrix((w, ci, rp), shape=(n, n))
    for scan in (False, True):
        counts = _u32(sir_counts(g, _state(p), edge_rates(g, M), gamma, sims, T, rng_seed=1234, edge_scan=scan))
        left = 1.0 - counts[0, -1].sum() / (sims * n)
        ratio = sigma_ratio(counts, sims, P)
        print(f"tree (scan={scan}): {left:.3f} of the (node, trajectory) pairs left S, largest |f - P| / bound unit = {ratio:.2f}")
        assert left > 0.25
        assert ratio <= 5.0
        folded = np.stack([p[:, 0] + p[:, 2], p[:, 1], np.zeros(n)], 1)        # an ignored immune set is NOT within the bound
        assert sigma_ratio(counts, sims, dmp_sir_init(rp, ci, w, gamma, folded, T, "float64")) > 5.0
    out = DMP_SIR(M, gamma).run(_state(p), T).cpu().numpy()
    o32 = dmp_sir_init(rp, ci, w, gamma, p, T, "float32")
    _check_bars("tree", out, o32, P, _rel(o32, P))


# ------------------------------------------------------------------ mean-field
def _meanfield(rp, ci, start, beta, gamma, maxTime):
    import scipy.sparse as sp
    from gnode import ode_nn
    n = len(rp) - 1
    A = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
    return ode_nn.runge_kutta_order4(ode_nn.sir, A, n, start, beta, gamma, 1, maxTime)


@pytest.mark.parametrize("n,m,gseed", [(700, 3000, 11), (257, 30, 12)], ids=["er700", "ragged-isolated"])
def test_meanfield_one_hot_state_is_the_seed_list_run(n, m, gseed, dev):
    from gnode.ode_nn import InitialState
    rp, ci, _ = _er(n, m, gseed)
    seeds = [0, n // 2]
    want = _meanfield(rp, ci, seeds, 0.05, 0.2, 9)
    got = _meanfield(rp, ci, InitialState.from_sets(n, seeds), 0.05, 0.2, 9)
    assert want[0][-1].max() > 0.01
    assert max(float(np.max(np.abs(a - b))) for a, b in zip(got, want)) <= 1e-12


@pytest.mark.parametrize("n,m,gseed,beta", [(700, 3000, 11, 0.05), (257, 30, 12, 0.4), (2001, 25000, 2, 0.002)], ids=["er700", "ragged-isolated", "hub"])
def test_meanfield_mixed_state(n, m, gseed, beta, dev):
    import gnode_oracle as O
    from sir_init_model import meanfield_init
    from sir_model import mixed_init
    rp, ci = O.chung_lu_graph(n, m, seed=gseed)[:2] if n == 2001 else _er(n, m, gseed)[:2]
    p, _ = mixed_init(n, 500 + n)
    got = _meanfield(rp, ci, _state(p), beta, 0.2, 8)
    want = meanfield_init(rp, ci, p, beta, 0.2, 8)
    diff = max(float(np.max(np.abs(a - b))) for a, b in zip(got, want))
    print(f"meanfield init n={n}: max |gpu - reference| = {diff:.3e}")
    assert diff <= MF_ATOL
    assert np.max(np.abs(got[0] + got[1] + got[2] - 1.0)) <= 1e-9
    assert np.array_equal(got[1][0], p[:, 0]) and np.array_equal(got[0][0], p[:, 1]) and np.array_equal(got[2][0], p[:, 2])
    assert np.max(np.abs(want[1][-1] - p[:, 0])) > 100 * MF_ATOL                # the case is not trivial
