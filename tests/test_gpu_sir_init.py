"""GPU: Monte-Carlo SIR labels from an initial-state distribution (gnode_sir_mc_philox_init through sir_counts /
sir_trajectories / sir_torch with an InitialState).  Every count comparison is np.array_equal on uint32 and runs for the
frontier walk and for edge_scan=True: against the seed-list calls where the state is one-hot, against the CPU model of
tests/sir_model.py on the cases of tests/sir_cases.py (held to the oracle by tests/test_sir_model.py) where it is not."""
import ctypes as C

import numpy as np
import pytest

from sir_cases import (IDS, INIT_SEED, INIT_SHAPES as SHAPES, case, dev, edge_weights, er_of, expected, graph, live_init, mixed_start,  # noqa: F401
                       state, u32)
from sir_model import one_way_path

pytestmark = pytest.mark.gpu


def _mixed_case(kind):
    """(rowptr, col, DeviceGraph, p, w, gamma) of the kind's mixed case: the inputs of `expected("init/<kind>")`."""
    c = case(f"init/{kind}")
    return c.rp, c.ci, graph(kind, c.n, c.m)[2], c.start, c.w, c.gamma


@pytest.mark.parametrize("kind,n,m,seeds,sims,T", SHAPES, ids=IDS)
def test_one_hot_state_equals_seed_list_call(kind, n, m, seeds, sims, T, dev):
    """One-hot I on the seed set, S elsewhere: the seed-list call's counts on rows t >= 1 and `sims` times its row 0, for
    the scalar, per-node and per-edge rate forms, sim_offset != 0."""
    from gnode.ode_nn import InitialState, sir_counts
    rp, ci, g = graph(kind, n, m)
    st = InitialState.from_sets(n, seeds)
    w, gamma = edge_weights(kind, n, len(ci), seeds)
    beta = np.random.default_rng(INIT_SEED[kind] + 50).uniform(0.05, 0.6, n)
    for name, b, gm in (("scalar", 0.45, 0.15), ("per-node", beta, gamma), ("per-edge", er_of(g, w), gamma), ("per-edge, scalar gamma", er_of(g, w), 0.2)):
        want = u32(sir_counts(g, seeds, b, gm, sims, T, rng_seed=11, sim_offset=5))
        assert want[1, 1:].any()
        for scan in (False, True):
            got = u32(sir_counts(g, st, b, gm, sims, T, rng_seed=11, sim_offset=5, edge_scan=scan))
            assert np.array_equal(got[:, 1:], want[:, 1:]), f"{kind}: {name}, scan={scan}: rows t >= 1"
            assert np.array_equal(got[:, 0], sims * want[:, 0]), f"{kind}: {name}, scan={scan}: row 0"


@pytest.mark.parametrize("kind,n,m,seeds,sims,T", SHAPES, ids=IDS)
def test_mixed_state_equals_cpu_model(kind, n, m, seeds, sims, T, dev):
    """Certain and uncertain rows with the per-edge weights and per-node gamma of the per-edge tests, against the CPU model:
    counts, events, curves, the events' counts and `counts=`."""
    import torch
    from gnode.ode_nn import sir_counts, sir_counts_from_events, sir_curves_from_events, sir_trajectories
    rp, ci, g, p, w, gamma = _mixed_case(kind)
    c, e = case(f"init/{kind}"), expected(f"init/{kind}")
    model = (e.counts, e.t_inf, e.t_rec)
    live_init(c, e)
    st, er = state(p), er_of(g, w)
    for scan in (False, True):
        counts = sir_counts(g, st, er, gamma, sims, T, rng_seed=21, edge_scan=scan)
        assert np.array_equal(u32(counts), model[0]), f"{kind}: counts != CPU model (scan={scan})"
        acc = torch.zeros_like(counts)
        tr = sir_trajectories(g, st, er, gamma, sims, T, rng_seed=21, counts=acc, edge_scan=scan)
        assert np.array_equal(tr.t_inf.cpu().numpy(), model[1]) and np.array_equal(tr.t_rec.cpu().numpy(), model[2]), f"{kind}: events (scan={scan})"
        assert torch.equal(sir_curves_from_events(tr.t_inf, tr.t_rec, T), tr.curves), f"{kind}: curves != sums of the events (scan={scan})"
        assert bool((tr.curves.sum(dim=2) == n).all())
        assert torch.equal(sir_counts_from_events(tr.t_inf, tr.t_rec, T, accumulate_t0=True), counts), f"{kind}: events -> counts (scan={scan})"
        assert torch.equal(acc, counts), f"{kind}: counts= of the trajectory call (scan={scan})"
        acc = sir_counts(g, st, er, gamma, sims, T, rng_seed=21, edge_scan=scan, counts=acc)
        assert np.array_equal(u32(acc), 2 * model[0]), f"{kind}: counts= accumulates (scan={scan})"


def test_other_rate_forms_with_a_mixed_state(dev):
    """The scalar and per-node forms of the init call (a constant and beta[col] in the model's per-position weights)."""
    from gnode.ode_nn import sir_counts
    n, sims, T = 503, 100, 10
    rp, ci, g = graph("er-small", n, 2500)
    p = mixed_start("er-small", n, rp)
    for name in ("scalar", "per-node", "per-node beta only"):
        c, want = case("init/forms-" + name), expected("init/forms-" + name).counts
        b, gm = c.beta, c.gamma
        assert want[1, -1].any() and want[2, -1].any()
        for scan in (False, True):
            assert np.array_equal(u32(sir_counts(g, state(p), b, gm, sims, T, rng_seed=33, sim_offset=4, edge_scan=scan)), want), f"{name}, scan={scan}"


def test_more_initially_infected_than_a_seed_list_carries(dev):
    """40 % of the wiki-vote-size nodes start infected (2 870 of 7 066, far past what a seed list is used for), another 10 %
    with probability 0.3: a first frontier that fills a large share of the uint16 lists."""
    from gnode.ode_nn import sir_counts
    n, sims, T = 7066, 32, 8
    rp, ci, g = graph("wiki-vote-size", n, 100736)
    p, want = case("init/many").start, expected("init/many").counts
    assert (p[:, 1] == 1.0).sum() > 0.39 * n
    assert want[1, 0].sum() > 0.39 * n * sims and want[0, -1].sum() < want[0, 0].sum()
    for scan in (False, True):
        assert np.array_equal(u32(sir_counts(g, state(p), 0.05, 0.1, sims, T, rng_seed=42, edge_scan=scan)), want), f"scan={scan}"


def test_nobody_susceptible(dev):
    """Every row I or R (crisp and uncertain): only recoveries happen -- the recovery-only branch from step 1 -- and the S
    counts are 0."""
    from gnode.ode_nn import sir_counts, sir_trajectories
    n, sims, T = 503, 100, 10
    rp, ci, g = graph("er-small", n, 2500)
    c, e = case("init/no-S"), expected("init/no-S")
    p, gamma, want = c.start, c.gamma, (e.counts, e.t_inf, e.t_rec)
    assert not want[0][0].any() and want[0][2, -1].sum() > want[0][2, 0].sum() and want[0][1, -1].any()
    for scan in (False, True):
        got = u32(sir_counts(g, state(p), np.full(n, 0.4), gamma, sims, T, rng_seed=51, edge_scan=scan))
        assert np.array_equal(got, want[0]), f"scan={scan}"
        tr = sir_trajectories(g, state(p), np.full(n, 0.4), gamma, sims, T, rng_seed=51, edge_scan=scan)
        assert bool((tr.t_inf == 0).all()) and np.array_equal(tr.t_rec.cpu().numpy(), want[2])
        assert bool((tr.curves[:, :, 0] == 0).all()) and bool((tr.curves.sum(dim=2) == n).all())


def test_nobody_infected(dev):
    """Every row S or R: nothing ever happens, all rows equal row 0 and the events are `never` or (0, 0)."""
    from gnode.ode_nn import sir_counts, sir_trajectories
    n, sims, T = 503, 100, 10
    rp, ci, g = graph("er-small", n, 2500)
    p, want = case("init/no-I").start, expected("init/no-I").counts
    for scan in (False, True):
        got = u32(sir_counts(g, state(p), 0.4, 0.2, sims, T, rng_seed=52, edge_scan=scan))
        assert np.array_equal(got, want), f"scan={scan}"
        assert np.array_equal(got, np.broadcast_to(got[:, :1], got.shape)) and not got[1].any()
        assert 0 < got[2, 0, 2::3].sum() < sims * len(got[2, 0, 2::3])
        tr = sir_trajectories(g, state(p), 0.4, 0.2, sims, T, rng_seed=52, edge_scan=scan)
        ti, trc = tr.t_inf.cpu().numpy(), tr.t_rec.cpu().numpy()
        assert np.array_equal(ti, trc) and set(np.unique(ti).tolist()) == {-1, 0}
        cv = tr.curves.cpu().numpy()
        assert np.array_equal(cv, np.broadcast_to(cv[:, :1], cv.shape)) and not cv[:, :, 1].any()


def test_single_row(dev):
    """T = 1: row 0 only."""
    from gnode.ode_nn import sir_trajectories
    import torch
    n, sims = 503, 100
    rp, ci, g = graph("er-small", n, 2500)
    p = mixed_start("er-small", n, rp)
    e = expected("init/T1")
    want = (e.counts, e.t_inf, e.t_rec)
    for scan in (False, True):
        acc = torch.zeros((3, 1, n), dtype=torch.int32, device=dev)
        tr = sir_trajectories(g, state(p), 0.3, 0.2, sims, 1, rng_seed=53, counts=acc, edge_scan=scan)
        assert np.array_equal(u32(acc), want[0]) and np.array_equal(tr.t_inf.cpu().numpy(), want[1])
        assert tr.curves.shape == (sims, 1, 3)
        assert np.array_equal(tr.curves[:, 0].cpu().numpy(), np.stack([(want[1] < 0).sum(1), ((want[1] == 0) & (want[2] < 0)).sum(1), (want[2] == 0).sum(1)], 1))


def test_immune_barrier(dev):
    """The one-way path 0 -> 1 -> ... -> 40 with certain transmission and no recovery, node 17 infected and node 25 immune:
    nodes 18 .. 24 are infected at steps 1 .. 7, nobody at or beyond the barrier ever is, and the barrier is R throughout."""
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import InitialState, sir_state_at, sir_trajectories
    n, rp, ci, w = one_way_path(40)
    g = DeviceGraph(rp, ci)
    sims, T = 33, 14
    want_inf = np.full(n, -1)
    want_inf[17:25] = np.arange(8)
    want_inf[25] = 0
    want_rec = np.full(n, -1)
    want_rec[25] = 0
    for scan in (False, True):
        tr = sir_trajectories(g, InitialState.from_sets(n, [17], immune=[25]), er_of(g, w), 0.0, sims, T, rng_seed=9, edge_scan=scan)
        assert np.array_equal(tr.t_inf.cpu().numpy(), np.broadcast_to(want_inf, (sims, n))), f"scan={scan}"
        assert np.array_equal(tr.t_rec.cpu().numpy(), np.broadcast_to(want_rec, (sims, n))), f"scan={scan}"
        for t in range(T):
            state = sir_state_at(tr.t_inf, tr.t_rec, t)
            assert bool((state[:, 25] == 2).all()) and not bool(state[:, 26:].any())


def test_sharded_equals_whole(dev):
    """Two shards of the sims range accumulated into one array equal one call, row 0 included."""
    import torch
    from gnode.ode_nn import sir_counts
    n, seeds = 503, [3, 499]
    rp, ci, g, p, w, gamma = _mixed_case("er-small")
    st, er = state(p), er_of(g, w)
    for scan in (False, True):
        whole = sir_counts(g, st, er, gamma, 1000, 12, rng_seed=5, edge_scan=scan)
        acc = sir_counts(g, st, er, gamma, 600, 12, rng_seed=5, sim_offset=0, edge_scan=scan)
        acc = sir_counts(g, st, er, gamma, 400, 12, rng_seed=5, sim_offset=600, counts=acc, edge_scan=scan)
        assert torch.equal(whole, acc)
        assert bool((whole.sum(dim=0) == 1000).all()) and whole[2, -1].sum().item() > whole[2, 0].sum().item()
    part = u32(sir_counts(g, st, er, gamma, 40, 12, rng_seed=5, sim_offset=600))
    assert np.array_equal(part, expected("init/shard").counts)


def test_large_state_paths(dev):
    """n = 100 000: the scan kernel keeps the trajectory state in memory, the frontier walk its lists (int32 ids)."""
    from gnode.ode_nn import sir_counts
    n, seeds = 100_000, [5, 77, 4242]
    rp, ci, g, p, w, gamma = _mixed_case("large")
    want = expected("init/large").counts
    assert (want[0, -1] < want[0, 0]).sum() > 1000
    st, er = state(p), er_of(g, w)
    assert np.array_equal(u32(sir_counts(g, st, er, gamma, 24, 8, rng_seed=99)), want)
    assert np.array_equal(u32(sir_counts(g, st, er, gamma, 24, 8, rng_seed=99, edge_scan=True)), want)


def test_fewer_entries_than_nodes_with_per_node_rates(dev):
    """`isolated` has fewer CSR entries than nodes: the per-node form's two arrays do not fit in front of the start
    thresholds, and the entry restates it per edge.  Same counts as the model's w = beta[col]."""
    from gnode.ode_nn import sir_counts
    n, sims, T = 300, 64, 6
    rp, ci, g = graph("isolated", n, 40)
    assert len(ci) < n
    c, want = case("init/isolated-nodes"), expected("init/isolated-nodes").counts
    p, beta, gamma = c.start, c.beta, c.gamma
    assert (want[0, -1] < want[0, 0]).any()
    for scan in (False, True):
        assert np.array_equal(u32(sir_counts(g, state(p), beta, gamma, sims, T, rng_seed=61, edge_scan=scan)), want), f"scan={scan}"


def test_seed_list_calls_untouched_after_init_calls(dev):
    """Nothing leaks through the handle or the workspace: seed-list calls of all three rate forms return after init calls
    what they returned before (the scalar one: the oracle's counts)."""
    import oracle_c as OC
    from gnode.ode_nn import sir_counts
    n, seeds = 503, [3, 499]
    rp, ci, g, p, w, gamma = _mixed_case("er-small")
    beta = np.random.default_rng(1).uniform(0.05, 0.6, n)
    forms = {"scalar": (0.3, 0.2), "per-node": (beta, gamma), "per-edge": (er_of(g, w), gamma)}
    before = {(k, scan): u32(sir_counts(g, seeds, b, gm, 64, 10, rng_seed=9, edge_scan=scan)) for k, (b, gm) in forms.items() for scan in (False, True)}
    for b, gm in forms.values():
        for scan in (False, True):
            sir_counts(g, state(p), b, gm, 64, 10, rng_seed=9, edge_scan=scan)
    for (k, scan), want in before.items():
        b, gm = forms[k]
        assert np.array_equal(u32(sir_counts(g, seeds, b, gm, 64, 10, rng_seed=9, edge_scan=scan)), want), f"{k}, scan={scan}"
    assert np.array_equal(before[("scalar", False)], OC.sir_philox(n, rp, ci, seeds, 0.3, 0.2, 64, 10, rng_seed=9))


def test_sir_torch_surface(dev):
    """An InitialState through the reference-shaped surface: row 0 holds counts and normalize_t0 has nothing to do."""
    from gnode.ode_nn import sir_torch
    c = case("init/karate")
    G, n, sims, T, p, gamma = c.G, c.n, c.sims, c.T, c.start, c.gamma
    want = expected("init/karate").counts.astype(np.float64)
    assert want[2, -1].sum() > want[2, 0].sum()
    for norm in (False, True):
        S, I, R = sir_torch(G, state(p), 0.3, gamma, sims, T, rng_seed=77, normalize_t0=norm)
        assert S.shape == (1, T, n) and S.dtype == np.float64
        assert np.array_equal(S[0], want[0]) and np.array_equal(I[0], want[1]) and np.array_equal(R[0], want[2])


def test_library_validates_the_state_and_the_rate_forms(dev):
    """The C entry checks every row itself (GNODE_ERR_ARG, the node in the message), refuses a workspace one byte short and
    the forbidden rate combinations, writes nothing when it refuses, and serves afterwards."""
    import torch
    from gnode import _lib
    lib = _lib.load()
    n, T, sims = 503, 6, 8
    rp, ci, g = graph("er-small", n, 2500)
    good = mixed_start("er-small", n, rp)
    counts = torch.zeros((3, T, n), dtype=torch.int32, device=dev)
    events = torch.full((2, sims, n), 7, dtype=torch.int16, device=dev)
    curves = torch.full((sims, T, 3), 7, dtype=torch.int32, device=dev)
    need = lib.gnode_sir_init_workspace_bytes(g.handle, T)
    assert need >= lib.gnode_sir_edges_workspace_bytes(g.handle, T) + 2 * 8 * n
    assert need < lib.gnode_sir_edges_workspace_bytes(g.handle, T) + 2 * 8 * n + 256
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rate, wgt = np.full(n, 0.2), np.full(len(ci), 0.3)
    hp = lambda a: None if a is None else _lib.host_ptr(a)

    def call(p, beta_host=None, w_host=None, gamma_host=None, nbytes=need, outputs=True):
        p = np.ascontiguousarray(p, dtype=np.float64)
        return lib.gnode_sir_mc_philox_init(g.handle, hp(p), 0.3, hp(beta_host), hp(w_host), 0.2, hp(gamma_host), sims, 0, T, C.c_uint64(1),
                                            _lib.ptr(events) if outputs else None, _lib.ptr(curves) if outputs else None,
                                            _lib.ptr(counts) if outputs else None, _lib.ptr(ws), nbytes, _lib.stream_ptr(), 0)

    for row in ((float("nan"), 0.5, 0.5), (-0.1, 0.6, 0.5), (1.5, 0.0, 0.0), (0.5, 0.3, 0.21)):
        p = good.copy()
        p[321] = row
        assert call(p) != 0 and "321" in lib.gnode_last_error().decode(), row
    assert call(good, nbytes=need - 1) != 0                                   # workspace one byte short
    assert call(good, beta_host=rate) != 0                                    # one per-node array without the other
    assert call(good, gamma_host=rate) != 0
    assert call(good, beta_host=rate, w_host=wgt) != 0                        # per-edge rates and a per-node beta
    assert call(good, beta_host=rate, w_host=wgt, gamma_host=rate) != 0
    assert call(good, outputs=False) != 0                                     # nothing to write
    bad_gamma = rate.copy()
    bad_gamma[77] = 2.0
    assert call(good, w_host=wgt, gamma_host=bad_gamma) != 0 and "77" in lib.gnode_last_error().decode()
    torch.cuda.synchronize()
    assert not counts.any() and bool((events == 7).all()) and bool((curves == 7).all())      # a refused call wrote nothing
    for kw in ({}, dict(beta_host=rate, gamma_host=rate), dict(w_host=wgt), dict(w_host=wgt, gamma_host=rate)):
        counts.zero_()
        assert call(good, **kw) == 0, lib.gnode_last_error().decode()          # ... and the handle still serves
        assert bool((counts.sum(dim=0) == sims).all())
