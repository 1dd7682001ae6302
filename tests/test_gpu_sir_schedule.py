"""GPU: the Monte-Carlo SIR with rates that change over time (gnode_sir_mc_philox_schedule through sir_counts /
sir_trajectories) against tests/sir_schedule_model.py, by INTEGER EQUALITY of counts, events and curves, on the cases of
tests/schedule_cases.py: three phases (the drawn weights, a closed phase, other weights and another gamma) with phase 0
revisited and a change at step T - 1, on every path of the kernels (lists in LDS, rows past GN_SIR_BIGROW, lists in the
workspace, the scan with its state in LDS and in memory, the everybody-infected branch).  tests/test_schedule_model.py runs
the cases' liveness checks on the CPU."""
import numpy as np
import pytest

import schedule_cases as K
import sir_cases as SC
import sir_model as M
from sir_cases import dev  # noqa: F401
from sir_schedule_model import schedule_thresholds, sir_events_schedule

pytestmark = pytest.mark.gpu


def _graph(c):
    if c.shape is not None:
        return SC.graph(*c.shape)[2]
    from gnode.graph import DeviceGraph
    return DeviceGraph(c.rp, c.ci)


def _schedules(c, g):
    from gnode.ode_nn import rate_schedule
    return (rate_schedule([SC.er_of(g, w) for w in c.W], steps=c.phase), rate_schedule(list(c.G), steps=c.phase))


def _start(c):
    return SC.state(c.start) if np.ndim(c.start) == 2 else c.start


def _run(c, dev, sims=None, sim_offset=None, counts=None, **kw):
    """(t_inf, t_rec, curves, counts) of a case through sir_trajectories, as host arrays"""
    import torch
    from gnode.ode_nn import sir_trajectories
    g = _graph(c)
    beta, gamma = _schedules(c, g)
    if counts is None:
        counts = torch.zeros((3, c.T, c.n), dtype=torch.int32, device=dev)
    r = sir_trajectories(g, _start(c), beta, gamma, c.sims if sims is None else sims, c.T, rng_seed=c.rng_seed,
                         sim_offset=c.sim_offset if sim_offset is None else sim_offset, counts=counts, device=dev, **kw)
    return r.t_inf.cpu().numpy(), r.t_rec.cpu().numpy(), SC.u32(r.curves), SC.u32(counts)


def _same(got, want):
    t_inf, t_rec, curves, counts = got
    assert np.array_equal(t_inf, want.t_inf) and np.array_equal(t_rec, want.t_rec)
    assert np.array_equal(curves, want.curves)
    assert np.array_equal(counts, want.counts)


@pytest.mark.parametrize("key", ["er-small/seeds", "er-small/init"])
@pytest.mark.parametrize("edge_scan", [False, True])
def test_er_small_all_outputs_both_kernels(key, edge_scan, dev):
    _same(_run(K.case(key), dev, edge_scan=edge_scan), K.expected(key))


@pytest.mark.parametrize("key", ["er-small/seeds", "er-small/init"])
def test_two_shards_add_up_to_the_whole(key, dev):
    import torch
    from gnode.ode_nn import sir_counts
    c, want = K.case(key), K.expected(key)
    g = _graph(c)
    beta, gamma = _schedules(c, g)
    cut = 77
    counts = torch.zeros((3, c.T, c.n), dtype=torch.int32, device=dev)
    a = _run(c, dev, sims=cut, sim_offset=0, counts=counts)
    b = _run(c, dev, sims=c.sims - cut, sim_offset=cut, counts=counts)
    assert np.array_equal(np.concatenate([a[0], b[0]]), want.t_inf) and np.array_equal(np.concatenate([a[1], b[1]]), want.t_rec)
    assert np.array_equal(np.concatenate([a[2], b[2]]), want.curves)
    assert np.array_equal(SC.u32(counts), want.counts)             # (the seed-list rule assigns row 0, a drawn start accumulates it)
    alone = sir_counts(g, _start(c), beta, gamma, c.sims, c.T, c.rng_seed, device=dev)     # counts alone: the instances without TRAJ
    assert np.array_equal(SC.u32(alone), want.counts)


@pytest.mark.parametrize("key,edge_scan", [("hubs/init", False), ("global-lists/init", False), ("large/init", True), ("large/init", False)])
def test_every_path_of_the_kernels(key, edge_scan, dev):
    from gnode import _lib
    c = K.case(key)
    kind = c.shape[0]
    if kind == "hubs":
        assert int(np.max(np.diff(c.rp))) > 512                    # rows past GN_SIR_BIGROW
    if kind == "global-lists":
        assert c.n > 11232                                         # the lists do not fit LDS
    if kind == "large":
        assert 2 * c.n > 150 * 1024                                # the scan's state does not fit LDS
    _same(_run(c, dev, edge_scan=edge_scan), K.expected(key))
    assert _lib.load().gnode_sir_schedule_workspace_bytes(_graph(c).handle, c.T, 3) > 3 * (len(c.ci) + c.n) * 8


def test_everybody_infected_recovers_at_the_switch(dev):
    """w = 1: from the step after the eccentricity the recovery-only branch runs, under gamma = 0 and then under gamma = 1"""
    c, want = K.case("everybody"), K.expected("everybody")
    for edge_scan in (False, True):
        got = _run(c, dev, edge_scan=edge_scan)
        _same(got, want)
        assert (got[1] == c.switch).all() and (got[2][:, c.switch] == (0, 0, c.n)).all()


# ----------------------------------------------------------------------------------------------------------------- karate
def _karate():
    G, n, rp, ci = SC.karate()
    from gnode.ode_nn import _device_graph_for
    return G, n, rp, ci, _device_graph_for(G)


def _model(n, rp, ci, start, W_by_step, G_by_step, sims, T, rng_seed, sim_offset=0):
    """the model with one phase per step: W_by_step[t - 1], G_by_step[t - 1] govern step t"""
    THR, TG = schedule_thresholds(W_by_step, G_by_step, len(ci), n)
    return sir_events_schedule(n, rp, ci, start, THR, TG, np.arange(-1, T - 1), sims, T, rng_seed, sim_offset)


def _check(r, counts, t_inf, t_rec, T, seeded):
    assert np.array_equal(r.t_inf.cpu().numpy(), t_inf) and np.array_equal(r.t_rec.cpu().numpy(), t_rec)
    assert np.array_equal(SC.u32(r.curves), M.curves(t_inf, t_rec, T))
    assert np.array_equal(SC.u32(counts), M.counts(t_inf, t_rec, T, hold_row0=seeded))


@pytest.mark.parametrize("T", [12, 2, 1])
def test_karate_one_phase_per_step(T, dev):
    """P = T - 1 (each step its own tables), T = 2 (one step) and T = 1 (no step: row 0 alone)"""
    import torch
    from gnode.ode_nn import rate_schedule, sir_trajectories
    G, n, rp, ci, g = _karate()
    rng = np.random.default_rng(50)
    P = max(T - 1, 1)
    W, Gm = rng.uniform(0.05, 0.9, (P, len(ci))), rng.uniform(0.05, 0.6, (P, n))
    W[:, ::7], Gm[:, 3] = 0.0, 1.0
    beta = rate_schedule([SC.er_of(g, w) for w in W], starts=range(1, P + 1))
    gamma = rate_schedule(list(Gm), starts=range(1, P + 1))
    p, _ = M.mixed_init(n, 34)
    for start, seeded in (([0, 33], True), (p, False)):
        counts = torch.zeros((3, T, n), dtype=torch.int32, device=dev)
        r = sir_trajectories(g, SC.state(start) if not seeded else start, beta, gamma, 300, T, rng_seed=77, sim_offset=9, counts=counts, device=dev)
        t_inf, t_rec = _model(n, rp, ci, start, list(W), list(Gm), 300, T, 77, 9)
        _check(r, counts, t_inf, t_rec, T, seeded)
        assert T < 12 or ((t_inf > 0).any() and (t_rec > 0).any())


def test_karate_mixed_forms_and_different_change_points(dev):
    """beta's values are a number, per-node rates and EdgeRates; gamma's a number and per-node rates, changing at other steps;
    sir_torch and sir_counts return the same counts"""
    import torch
    from gnode.ode_nn import rate_schedule, sir_counts, sir_torch, sir_trajectories
    G, n, rp, ci, g = _karate()
    T = 12
    rng = np.random.default_rng(51)
    b_node, w_edge, g_node = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.9, len(ci)), rng.uniform(0.05, 0.6, n)
    b_node[[4, 20]], w_edge[::5] = 0.0, 0.0
    beta = rate_schedule([0.3, b_node, SC.er_of(g, w_edge)], starts=[1, 4, 8])
    gamma = rate_schedule([0.2, g_node], steps=[0, 0, 0, 1, 1, 1, 0, 0, 1, 1, 0, 1])
    B = [np.full(len(ci), 0.3), b_node[ci], w_edge]
    Gv = [np.full(n, 0.2), g_node]
    W_by_step = [B[beta.phase_of_step(T)[t]] for t in range(1, T)]
    G_by_step = [Gv[gamma.phase_of_step(T)[t]] for t in range(1, T)]
    t_inf, t_rec = _model(n, rp, ci, [0, 33], W_by_step, G_by_step, 300, T, 77)
    assert (t_inf > 0).mean() > 0.25
    counts = torch.zeros((3, T, n), dtype=torch.int32, device=dev)
    r = sir_trajectories(g, [0, 33], beta, gamma, 300, T, rng_seed=77, counts=counts, device=dev)
    _check(r, counts, t_inf, t_rec, T, True)
    want = M.counts(t_inf, t_rec, T, hold_row0=True)
    assert np.array_equal(SC.u32(sir_counts(g, [0, 33], beta, gamma, 300, T, 77, device=dev)), want)
    S, I, R = sir_torch(G, [0, 33], beta, gamma, sims=300, T=T, rng_seed=77)
    assert np.array_equal(np.stack([S[0], I[0], R[0]]), want.astype(np.float64))


@pytest.mark.parametrize("form", ["scalar", "nodes", "edges"])
def test_karate_one_phase_is_the_constant_call(form, dev):
    import torch
    from gnode.ode_nn import rate_schedule, sir_trajectories
    G, n, rp, ci, g = _karate()
    T, sims = 12, 200
    rng = np.random.default_rng(52)
    beta, gamma = {"scalar": (0.3, 0.2), "nodes": (rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)),
                   "edges": (SC.er_of(g, rng.uniform(0.05, 0.9, len(ci))), rng.uniform(0.05, 0.6, n))}[form]
    p, _ = M.mixed_init(n, 34)
    for start in ([0, 33], SC.state(p)):
        outs = []
        for b, gm in ((beta, gamma), (rate_schedule([beta], starts=[1]), rate_schedule([gamma], starts=[1])),
                      (rate_schedule([beta, beta], starts=[1, 5]), gamma)):
            counts = torch.zeros((3, T, n), dtype=torch.int32, device=dev)
            r = sir_trajectories(g, start, b, gm, sims, T, rng_seed=5, sim_offset=3, counts=counts, device=dev)
            outs.append((r.t_inf, r.t_rec, r.curves, counts))
        assert bool((outs[0][0] > 0).any()) and bool((outs[0][1] > 0).any())
        for other in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(outs[0], other))


def test_the_entry_refuses_and_writes_nothing(dev):
    """through the C entry: P < 1, a phase out of range, a rate out of range (phase and position named), both and neither
    kind of start, a short workspace; the outputs keep their fill, and a good call after them is served"""
    import ctypes as C
    import torch
    from gnode import _lib
    G, n, rp, ci, g = _karate()
    lib = _lib.load()
    ARG, WORKSPACE = -1, -3
    T, P, sims, nnz = 6, 2, 8, len(ci)
    rng = np.random.default_rng(53)
    W, Gm = np.ascontiguousarray(rng.uniform(0.05, 0.9, (P, nnz))), np.ascontiguousarray(rng.uniform(0.05, 0.6, (P, n)))
    phase = np.asarray([0, 0, 1, 1, 0, 1], dtype=np.int32)
    seeds = np.asarray([0, 33], dtype=np.int32)
    init = np.ascontiguousarray(M.mixed_init(n, 34)[0])
    need = lib.gnode_sir_schedule_workspace_bytes(g.handle, T, P)
    assert lib.gnode_sir_schedule_workspace_bytes(g.handle, T, 0) == 0 and lib.gnode_sir_schedule_workspace_bytes(None, T, P) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ev = torch.full((2, sims, n), 7, dtype=torch.int16, device=dev)
    cv = torch.full((sims, T, 3), 7, dtype=torch.int32, device=dev)
    cnt = torch.full((3, T, n), 7, dtype=torch.int32, device=dev)

    def call(seeds=seeds, n_seeds=2, init=None, phase=phase, P=P, W=W, Gm=Gm, nbytes=need, outs=(ev, cv, cnt)):
        hp = lambda a: None if a is None else _lib.host_ptr(a)      # noqa: E731
        return lib.gnode_sir_mc_philox_schedule(g.handle, hp(seeds), n_seeds, hp(init), hp(phase), P, hp(W), hp(Gm), sims, 0, T, C.c_uint64(11),
                                                *(_lib.ptr(o) for o in outs), _lib.ptr(ws), nbytes, _lib.stream_ptr(), 0)

    said = lambda: lib.gnode_last_error().decode()                  # noqa: E731
    assert call(P=0) == ARG
    bad = phase.copy(); bad[4] = 2
    assert call(phase=bad) == ARG and "phase[4] = 2" in said()
    bad = phase.copy(); bad[0] = 99                                 # entry 0 is never read
    x = W.copy(); x[1, 17] = 1.25
    assert call(W=x) == ARG and "phase 1" in said() and "position 17" in said()
    x = Gm.copy(); x[0, 5] = float("nan")
    assert call(Gm=x) == ARG and "phase 0" in said() and "gamma[5]" in said()
    assert call(init=init) == ARG                                   # both kinds of start
    assert call(seeds=None, n_seeds=0) == ARG                       # neither
    assert call(outs=(None, None, None)) == ARG
    assert call(nbytes=need - 1) == WORKSPACE
    torch.cuda.synchronize()
    assert bool((ev == 7).all()) and bool((cv == 7).all()) and bool((cnt == 7).all())
    cnt.zero_()
    assert call(phase=bad) == 0, said()
    THR, TG = schedule_thresholds(list(W), list(Gm), nnz, n)
    t_inf, t_rec = sir_events_schedule(n, rp, ci, [0, 33], THR, TG, phase, sims, T, 11)
    assert np.array_equal(ev[0].cpu().numpy(), t_inf) and np.array_equal(ev[1].cpu().numpy(), t_rec)
    assert np.array_equal(SC.u32(cnt), M.counts(t_inf, t_rec, T, hold_row0=True))
    cnt.zero_()
    assert call(seeds=None, n_seeds=0, init=init) == 0, said()     # the drawn start through the same entry
    t_inf, t_rec = sir_events_schedule(n, rp, ci, init, THR, TG, phase, sims, T, 11)
    assert np.array_equal(ev[0].cpu().numpy(), t_inf) and np.array_equal(SC.u32(cnt), M.counts(t_inf, t_rec, T, hold_row0=False))
