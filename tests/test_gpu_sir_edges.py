"""GPU: Monte-Carlo SIR labels with per-edge transmission probabilities (gnode_sir_mc_philox_edges / _traj_edges through
sir_counts / sir_trajectories / sir_torch with an EdgeRates).  Every comparison but the last is np.array_equal on uint32
counts: against the scalar call where the weights are one constant, against the per-node call where w[p] = beta[col[p]],
against the CPU model of tests/sir_model.py on the cases of tests/sir_cases.py (held to the oracle by
tests/test_sir_model.py) where they are neither.  The last holds the counts to DMP's marginals on a tree, where those are
exact: the direction convention."""
import numpy as np
import pytest

from baseline_cases import rel as _rel
from sir_cases import (EDGE_RATE_SEED, IDS, SHAPES, bfs_depth, case, dev, dmp_ratio, edge_weights, er_of, expected, graph,  # noqa: F401
                       live_edges, tree_case, u32)
from sir_model import one_way_path

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,n,m,seeds,sims,T", SHAPES, ids=IDS)
def test_constant_weights_equal_scalar_call(kind, n, m, seeds, sims, T, dev):
    """One constant on every entry returns the scalar call's counts, bit for bit: frontier walk and edge scan, scalar and
    per-node gamma, sim_offset != 0."""
    from gnode.ode_nn import sir_counts
    rp, ci, g = graph(kind, n, m)
    for beta, gamma, rs in ((0.45, 0.15, 11), (0.05, 0.6, 12)):
        want = u32(sir_counts(g, seeds, beta, gamma, sims, T, rng_seed=rs, sim_offset=5))
        assert want[1, 1:].any()
        er = er_of(g, np.full(len(ci), beta))
        for scan in (False, True):
            for gm in (gamma, np.full(n, gamma)):
                got = u32(sir_counts(g, seeds, er, gm, sims, T, rng_seed=rs, sim_offset=5, edge_scan=scan))
                assert np.array_equal(got, want), f"{kind}: per-edge call with a constant != scalar call (beta={beta}, scan={scan})"


@pytest.mark.parametrize("kind,n,m,seeds,sims,T", SHAPES, ids=IDS)
def test_target_weights_equal_per_node_call(kind, n, m, seeds, sims, T, dev):
    """w[p] = beta[col[p]] with per-node gamma returns the per-node call's counts."""
    from gnode.ode_nn import sir_counts
    rp, ci, g = graph(kind, n, m)
    rng = np.random.default_rng(EDGE_RATE_SEED[kind] + 50)
    beta, gamma = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
    beta[rng.permutation(n)[:n // 10]] = 0.0
    want = u32(sir_counts(g, seeds, beta, gamma, sims, T, rng_seed=13, sim_offset=2))
    assert want[1, 1:].any()
    er = er_of(g, beta[ci])
    for scan in (False, True):
        got = u32(sir_counts(g, seeds, er, gamma, sims, T, rng_seed=13, sim_offset=2, edge_scan=scan))
        assert np.array_equal(got, want), f"{kind}: w = beta[col] != per-node call (scan={scan})"


@pytest.mark.parametrize("kind,n,m,seeds,sims,T", SHAPES, ids=IDS)
def test_heterogeneous_weights_equal_cpu_model(kind, n, m, seeds, sims, T, dev):
    """Frontier walk and edge scan with a different, asymmetric weight on every directed entry, closed (w = 0) and certain
    (w = 1) entries among them, per-node gamma, against the CPU model.  The model's output is first checked for a live
    epidemic, so that two dead ones cannot pass for agreement."""
    from gnode.ode_nn import sir_counts
    g = graph(kind, n, m)[2]
    c, model = case(f"edges/{kind}"), expected(f"edges/{kind}")
    seeds, w, gamma = c.start, c.w, c.gamma
    live_edges(c, model)
    er = er_of(g, w)
    a = u32(sir_counts(g, seeds, er, gamma, sims, T, rng_seed=21))
    assert np.array_equal(a, model.counts), f"{kind}: frontier walk != CPU model"
    b = u32(sir_counts(g, seeds, er, gamma, sims, T, rng_seed=21, edge_scan=True))
    assert np.array_equal(b, model.counts), f"{kind}: edge scan != CPU model"


def test_large_state_paths(dev):
    """n = 100 000: the scan kernel keeps the trajectory state in memory, the frontier walk its lists (int32 ids)."""
    from gnode.ode_nn import sir_counts
    c, want = case("edges/large"), expected("edges/large").counts
    g, seeds, w, gamma = graph("large", c.n, c.m)[2], c.start, c.w, c.gamma
    assert (want[0, -1] < 24).sum() > 1000
    er = er_of(g, w)
    assert np.array_equal(u32(sir_counts(g, seeds, er, gamma, 24, 8, rng_seed=99)), want)
    assert np.array_equal(u32(sir_counts(g, seeds, er, gamma, 24, 8, rng_seed=99, edge_scan=True)), want)


def test_one_way_path(dev):
    """w = 1 on every entry i -> i + 1, 0 on every i + 1 -> i, gamma = 0, seed in the middle m: node m + j is infected at
    step j in every trajectory and nobody below m ever is.  Fails if the weight of the reverse entry, or a weight chosen
    by the target node, is used."""
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import sir_trajectories
    k, m, sims = 40, 17, 33
    n, rp, ci, w = one_way_path(k)
    g = DeviceGraph(rp, ci)
    T = k - m + 3
    want = np.full(n, -1)
    want[m:] = np.arange(n - m)
    for scan in (False, True):
        tr = sir_trajectories(g, [m], er_of(g, w), 0.0, sims, T, rng_seed=9, edge_scan=scan)
        assert np.array_equal(tr.t_inf.cpu().numpy(), np.broadcast_to(want, (sims, n))), f"scan={scan}"
        assert bool((tr.t_rec == -1).all())


def test_more_than_32_seeds(dev):
    """40 seeds: the list is copied from the host instead of travelling as a kernel argument."""
    from gnode.ode_nn import sir_counts
    c, want = case("edges/seeds40"), expected("edges/seeds40").counts
    g, seeds, w, gamma = graph("er-small", c.n, c.m)[2], c.start, c.w, c.gamma
    assert len(seeds) == 40 and max(seeds) < c.n
    er = er_of(g, w)
    assert np.array_equal(u32(sir_counts(g, seeds, er, gamma, 50, 8, rng_seed=31)), want)
    assert np.array_equal(u32(sir_counts(g, seeds, er, gamma, 50, 8, rng_seed=31, edge_scan=True)), want)


def test_sharded_equals_whole(dev):
    """Two shards of the sims range accumulated into one array equal one call."""
    import torch
    from gnode.ode_nn import sir_counts
    n, seeds = 500, [3, 499]
    rp, ci, g = graph("er-small", n, 2500)
    w, gamma = edge_weights("er-small", n, len(ci), seeds)
    er = er_of(g, w)
    whole = sir_counts(g, seeds, er, gamma, 1000, 12, rng_seed=5)
    acc = sir_counts(g, seeds, er, gamma, 600, 12, rng_seed=5, sim_offset=0)
    acc = sir_counts(g, seeds, er, gamma, 400, 12, rng_seed=5, sim_offset=600, counts=acc)
    assert torch.equal(whole, acc)
    assert whole[2, -1].sum().item() > 0
    # the second shard alone is the model's trajectories 600..639
    part = u32(sir_counts(g, seeds, er, gamma, 40, 12, rng_seed=5, sim_offset=600))
    assert np.array_equal(part, expected("edges/shard").counts)


def test_extreme_weights(dev):
    """w = 0 everywhere leaves only the seed infected; w = 1 everywhere with gamma = 0 infects exactly the BFS ball of
    radius t (the threshold 2^32 of p = 1 does not fit 32 bits)."""
    from gnode.ode_nn import sir_counts
    n, seed, sims = 300, 11, 32
    rp, ci, g = graph("er300", n, 600)
    depth = bfs_depth(rp, ci, seed, n)
    comp, ecc = depth >= 0, int(depth.max())
    assert comp.sum() > 200 and ecc >= 4
    T = ecc + 2
    ones, zeros = er_of(g, np.ones(len(ci))), er_of(g, np.zeros(len(ci)))
    for scan in (False, True):
        got = u32(sir_counts(g, [seed], ones, 0.0, sims, T, rng_seed=3, edge_scan=scan))
        for t in range(1, T):
            assert np.array_equal(got[1, t], np.where(comp & (depth <= t), sims, 0)), t
        assert np.all(got[1, ecc][comp] == sims) and not got[2].any()
        got0 = u32(sir_counts(g, [seed], zeros, np.full(n, 0.3), sims, T, rng_seed=3, edge_scan=scan))
        others = np.arange(n) != seed
        assert np.all(got0[0, 1:][:, others] == sims) and np.all(got0[0, 1:, seed] == 0)
        assert got0[2, -1, seed] > 0


@pytest.mark.parametrize("kind,n,m,seeds,sims,T", [SHAPES[0], SHAPES[2], SHAPES[3]], ids=[IDS[i] for i in (0, 2, 3)])
def test_trajectories_consistent_with_counts(kind, n, m, seeds, sims, T, dev):
    """sir_counts_from_events of the per-edge trajectory call equals the per-edge counts call, the events equal the CPU
    model's, the curves are the events' sums and `counts=` accumulates what sir_counts adds."""
    import torch
    from gnode.ode_nn import sir_counts, sir_counts_from_events, sir_curves_from_events, sir_trajectories
    g = graph(kind, n, m)[2]
    c, model = case(f"edges/{kind}"), expected(f"edges/{kind}")       # (these kinds' heterogeneous case starts from the shape's seeds)
    assert c.start == seeds
    w, gamma, t_inf, t_rec = c.w, c.gamma, model.t_inf, model.t_rec
    er = er_of(g, w)
    want = sir_counts(g, seeds, er, gamma, sims, T, rng_seed=21)
    for scan in (False, True):
        acc = torch.zeros_like(want)
        tr = sir_trajectories(g, seeds, er, gamma, sims, T, rng_seed=21, counts=acc, edge_scan=scan)
        assert torch.equal(sir_counts_from_events(tr.t_inf, tr.t_rec, T), want), f"{kind}: events -> counts != sir_counts (scan={scan})"
        assert torch.equal(acc, want), f"{kind}: counts= of the trajectory call != sir_counts (scan={scan})"
        assert torch.equal(sir_curves_from_events(tr.t_inf, tr.t_rec, T), tr.curves), f"{kind}: curves != sums of the events"
        assert bool((tr.curves.sum(dim=2) == n).all())
        assert np.array_equal(tr.t_inf.cpu().numpy(), t_inf) and np.array_equal(tr.t_rec.cpu().numpy(), t_rec)


def test_sir_torch_surface(dev):
    """An EdgeRates made from a networkx graph and a scipy matrix, through the reference-shaped surface."""
    import scipy.sparse as sp
    from gnode.ode_nn import edge_rates, sir_torch
    c = case("edges/karate")
    G, n, rp, ci, sims, T, seeds, w, gamma, keep = c.G, c.n, c.rp, c.ci, c.sims, c.T, c.start, c.w, c.gamma, c.keep
    src = np.repeat(np.arange(n), np.diff(rp))
    M = sp.coo_matrix((w[keep], (src[keep], ci[keep])), shape=(n, n))   # the zeros are absent from the matrix, the rest shuffled
    want = expected("edges/karate").counts.astype(np.float64)
    assert want[2, -1].sum() > 0
    S, I, R = sir_torch(G, seeds, edge_rates(G, M), gamma, sims, T, rng_seed=77)
    assert S.shape == (1, T, n) and S.dtype == np.float64
    assert np.array_equal(S[0], want[0]) and np.array_equal(I[0], want[1]) and np.array_equal(R[0], want[2])
    S1, I1, R1 = sir_torch(G, seeds, edge_rates(G, M.tocsr()), gamma.tolist(), sims, T, rng_seed=77, normalize_t0=True)
    want[:, 0] *= sims
    assert np.array_equal(S1[0], want[0]) and np.array_equal(I1[0], want[1]) and np.array_equal(R1[0], want[2])


def test_other_forms_untouched_after_per_edge_calls(dev):
    """No state leaks through the handle or the workspace: scalar and per-node calls after per-edge calls return what they
    returned before (the scalar one: the oracle's counts)."""
    import oracle_c as OC
    from gnode.ode_nn import sir_counts
    n, seeds = 500, [3, 499]
    rp, ci, g = graph("er-small", n, 2500)
    w, gamma = edge_weights("er-small", n, len(ci), seeds)
    beta = np.random.default_rng(1).uniform(0.05, 0.6, n)
    before = {scan: u32(sir_counts(g, seeds, beta, gamma, 64, 10, rng_seed=9, edge_scan=scan)) for scan in (False, True)}
    er = er_of(g, w)
    sir_counts(g, seeds, er, gamma, 64, 10, rng_seed=9)
    sir_counts(g, seeds, er, 0.2, 64, 10, rng_seed=9, edge_scan=True)
    for scan in (False, True):
        got = u32(sir_counts(g, seeds, 0.3, 0.2, 64, 10, rng_seed=9, edge_scan=scan))
        assert np.array_equal(got, OC.sir_philox(n, rp, ci, seeds, 0.3, 0.2, 64, 10, rng_seed=9))
        assert np.array_equal(u32(sir_counts(g, seeds, beta, gamma, 64, 10, rng_seed=9, edge_scan=scan)), before[scan])


def test_counts_agree_with_dmp_on_a_tree(dev):
    """On a tree DMP's marginals are the exact ones, and gnode_dmp_f32 / O.dmp_sir read `weights` as source = row, target
    = column: 20 000 trajectories lie within the project's per-cell 5 sigma bound of them,
    |count / sims - P| <= 5 (sqrt(P (1 - P) / sims) + 1 / sims), in every cell of rows t >= 1.  A condition, not a
    measurement: the CPU model gives a largest ratio of about 3 whatever the number of trajectories, and the GPU counts
    are the model's bit for bit, so a failure here is a wrong convention, not noise."""
    import gnode_oracle as O
    import scipy.sparse as sp
    from gnode.dmp import DMP_SIR
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import edge_rates, sir_counts
    n, rp, ci, w, gamma = tree_case()
    sims, T = 20000, 12
    P = O.dmp_sir(rp, ci, w, gamma, [0], T, dtype="float64")
    g = DeviceGraph(rp, ci)
    M = sp.csr_matrix((w, ci, rp), shape=(n, n))
    counts = u32(sir_counts(g, [0], edge_rates(g, M), gamma, sims, T, rng_seed=1234))
    left = 1.0 - counts[0, -1].sum() / (sims * n)
    ratio = dmp_ratio(counts, sims, P)
    print(f"tree: {left:.3f} of the (node, trajectory) pairs left S, largest |f - P| / bound unit = {ratio:.2f}")
    assert left > 0.25
    assert ratio <= 5.0
    # the transposed reading of the same weights is NOT within the bound: the test can tell the conventions apart
    assert dmp_ratio(counts, sims, O.dmp_sir(rp, ci, edge_rates(g, sp.csr_matrix(M.T)).w, gamma, [0], T, dtype="float64")) > 5.0
    # gnode_dmp_f32 on the same matrix, at test_gpu_baselines.py's fp32 tolerances against the oracle
    out = DMP_SIR(M, gamma).run([0], T).cpu().numpy()
    o32 = O.dmp_sir(rp, ci, w, gamma, [0], T)
    yard = _rel(o32, P)
    assert _rel(out, o32) <= 1e-5
    assert _rel(out, P) <= max(4 * yard, 1e-6)


def test_library_validates_weights_and_takes_an_empty_graph(dev):
    """The C entry checks every weight itself (GNODE_ERR_ARG, the CSR position in the message) and accepts a NULL array
    for a graph without entries."""
    import ctypes as C
    import torch
    from gnode import _lib
    from gnode.graph import DeviceGraph
    lib = _lib.load()
    n = 500
    rp, ci, g = graph("er-small", n, 2500)
    T, seeds = 6, np.array([3], np.int32)
    counts = torch.zeros((3, T, n), dtype=torch.int32, device=dev)
    ws = torch.empty(lib.gnode_sir_edges_workspace_bytes(g.handle, T), dtype=torch.uint8, device=dev)
    assert ws.numel() >= lib.gnode_sir_workspace_bytes(g.handle, T) + 8 * (len(ci) + n)

    def call(graph, w, gamma_host, nbytes, n_nodes):
        c = counts if n_nodes == n else torch.zeros((3, T, n_nodes), dtype=torch.int32, device=dev)
        return lib.gnode_sir_mc_philox_edges(graph.handle, _lib.host_ptr(seeds), 1, None if w is None else _lib.host_ptr(w), 0.2,
                                             None if gamma_host is None else _lib.host_ptr(gamma_host), 8, 0, T, C.c_uint64(1),
                                             _lib.ptr(c), _lib.ptr(ws), nbytes, _lib.stream_ptr(), 0), c

    for bad in (-0.25, 1.5, float("nan")):
        w = np.full(len(ci), 0.3)
        w[1234] = bad
        status, _ = call(g, w, None, ws.numel(), n)
        assert status != 0 and "1234" in lib.gnode_last_error().decode()
    gam = np.full(n, 0.2)
    gam[77] = 2.0
    assert call(g, np.full(len(ci), 0.3), gam, ws.numel(), n)[0] != 0 and "77" in lib.gnode_last_error().decode()
    assert call(g, None, None, ws.numel(), n)[0] != 0                                   # NULL weights with nnz > 0
    assert call(g, np.full(len(ci), 0.3), None, ws.numel() - 1, n)[0] != 0              # workspace one byte short
    assert not counts.any()                                                             # a refused call wrote nothing
    assert call(g, np.full(len(ci), 0.3), None, ws.numel(), n)[0] == 0                  # ... and the handle still serves
    # no entries: NULL is accepted and the seed recovers on its own
    g0 = DeviceGraph(np.zeros(6, np.int32), np.zeros(0, np.int32))
    status, c0 = call(g0, None, None, ws.numel(), 5)
    assert status == 0, lib.gnode_last_error().decode()
    c0 = u32(c0)
    assert np.all(c0[0, 1:, [0, 1, 2, 4]] == 8) and np.all(c0[0, 1:, 3] == 0) and np.all(c0[1, 1:, 3] + c0[2, 1:, 3] == 8)
