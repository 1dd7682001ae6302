"""GPU: per-trajectory Monte-Carlo SIR output (gnode_sir_mc_philox_traj through gnode.ode_nn.sir_trajectories): the step at
which every node of every trajectory was infected and recovered, and each trajectory's population totals.  Every
comparison is array_equal on integers: against the CPU model of tests/sir_model.py on the cases of tests/sir_cases.py (held
to the oracle by tests/test_sir_model.py), against the production call `sir_counts`, and between the two kernels.  Shapes,
graphs and rates are those of tests/test_gpu_sir_nodes.py: the smallest that reach each storage form."""
import numpy as np
import pytest

from sir_cases import IDS, SHAPE, SHAPES, bfs_depth, case, dev, expected, graph, live_events, node_rates  # noqa: F401
from sir_model import states_at

pytestmark = pytest.mark.gpu


def _np(tr):
    """(t_inf, t_rec, curves) of a SirTrajectories on the host; curves as the kernel's uint32."""
    return tr.t_inf.cpu().numpy(), tr.t_rec.cpu().numpy(), tr.curves.cpu().numpy().astype(np.uint32)


def _want(key):
    """(t_inf, t_rec, curves) of the model on a case of sir_cases."""
    e = expected(key)
    return e.t_inf, e.t_rec, e.curves


def _same(got, want, what, rows=None):
    for name, a, b in zip(("t_inf", "t_rec", "curves"), got, want):
        a = a if rows is None else a[:rows]
        assert a.dtype == b.dtype and np.array_equal(a, b), f"{what}: {name} differs"


# -------------------------------------------------------------------------------------------------- 1. against the CPU model
MODEL_SIMS = {"wiki-vote-size": 24}       # the model runs the first 24 trajectories only there (the CPU side stays short)


@pytest.mark.parametrize("kind,n,m,seeds,sims,T", SHAPES, ids=IDS)
def test_events_and_curves_equal_cpu_model(kind, n, m, seeds, sims, T, dev):
    from gnode.ode_nn import sir_trajectories
    g = graph(kind, n, m)[2]
    msims = MODEL_SIMS.get(kind, sims)
    key = f"nodes/{kind}" + (f"/{msims}" if msims != sims else "")
    c, want = case(key), _want(key)
    seeds, beta, gamma = c.start, c.beta, c.gamma
    live_events(c, expected(key))
    for scan in (False, True):
        tr = sir_trajectories(g, seeds, beta, gamma, sims, T, rng_seed=21, edge_scan=scan)
        assert tr.t_inf.shape == (sims, n) and tr.t_rec.shape == (sims, n) and tr.curves.shape == (sims, T, 3)
        _same(_np(tr), want, f"{kind}, edge_scan={scan}", rows=msims)


# -------------------------------------------------------------------------------------------------- 2. scalar rates, sim_offset
@pytest.mark.parametrize("kind,n,m,seeds,sims,T", SHAPES, ids=IDS)
def test_scalar_rates_equal_constant_arrays(kind, n, m, seeds, sims, T, dev):
    from gnode.ode_nn import sir_trajectories
    rp, ci, g = graph(kind, n, m)
    for beta, gamma, rs in ((0.45, 0.15, 11), (0.05, 0.6, 12)):
        a = _np(sir_trajectories(g, seeds, beta, gamma, sims, T, rng_seed=rs, sim_offset=5))
        b = _np(sir_trajectories(g, seeds, np.full(n, beta), np.full(n, gamma), sims, T, rng_seed=rs, sim_offset=5))
        _same(b, a, f"{kind}: constant arrays != scalar rates (beta={beta})")
        c = _np(sir_trajectories(g, seeds, beta, [gamma] * n, sims, T, rng_seed=rs, sim_offset=5, edge_scan=True))
        _same(c, a, f"{kind}: edge scan with an array gamma != scalar rates (beta={beta})")


# -------------------------------------------------------------------------------------------------- 3. the production call
def _check_identities(g, seeds, beta, gamma, sims, T, rs, what, edge_scan=False):
    """events -> counts == sir_counts, events -> curves == the kernel's curves, counts= == sir_counts.  Returns the result."""
    import torch
    from gnode.ode_nn import sir_counts, sir_counts_from_events, sir_curves_from_events, sir_trajectories
    want = sir_counts(g, seeds, beta, gamma, sims, T, rng_seed=rs, sim_offset=2)
    acc = torch.zeros_like(want)
    tr = sir_trajectories(g, seeds, beta, gamma, sims, T, rng_seed=rs, sim_offset=2, counts=acc, edge_scan=edge_scan)
    assert torch.equal(acc, want), f"{what}: counts= of sir_trajectories != sir_counts"
    from_ev = sir_counts_from_events(tr.t_inf, tr.t_rec, T)
    assert from_ev.dtype == torch.int32 and torch.equal(from_ev, want), f"{what}: sir_counts_from_events != sir_counts"
    cv = sir_curves_from_events(tr.t_inf, tr.t_rec, T)
    assert cv.dtype == torch.int32 and torch.equal(cv, tr.curves), f"{what}: sir_curves_from_events != curves"
    both = (tr.t_inf >= 0) & (tr.t_rec >= 0)
    assert bool((tr.t_rec[both] > tr.t_inf[both]).all())
    return tr


@pytest.mark.parametrize("kind,n,m,seeds,sims,T", SHAPES, ids=IDS)
def test_consistent_with_production_call(kind, n, m, seeds, sims, T, dev):
    rp, ci, g = graph(kind, n, m)
    beta, gamma, _ = node_rates(kind, n, seeds)
    _check_identities(g, seeds, 0.3, 0.2, sims, T, 9, f"{kind}, scalar rates")
    _check_identities(g, seeds, beta, gamma, sims, T, 9, f"{kind}, per-node rates")


def test_scalar_production_call_untouched_after_traj_calls(dev):
    import oracle_c as OC
    from gnode.ode_nn import sir_counts, sir_trajectories
    kind, n, m, seeds, sims, T = SHAPE["er-small"]
    rp, ci, g = graph(kind, n, m)
    beta, gamma, _ = node_rates(kind, n, seeds)
    sir_trajectories(g, seeds, beta, gamma, 64, 10, rng_seed=9)
    sir_trajectories(g, seeds, 0.3, 0.2, 64, 10, rng_seed=9, edge_scan=True)
    for scan in (False, True):
        got = sir_counts(g, seeds, 0.3, 0.2, 64, 10, rng_seed=9, edge_scan=scan).cpu().numpy().astype(np.uint32)
        assert np.array_equal(got, OC.sir_philox(n, rp, ci, seeds, 0.3, 0.2, 64, 10, rng_seed=9))


# -------------------------------------------------------------------------------------------------- 4. one output at a time
@pytest.mark.parametrize("kind", ["er-small", "global-lists"])
@pytest.mark.parametrize("scan", [False, True], ids=["frontier", "scan"])
def test_one_output_at_a_time(kind, scan, dev):
    import torch
    from gnode.ode_nn import sir_trajectories
    _, n, m, seeds, sims, T = SHAPE[kind]
    rp, ci, g = graph(kind, n, m)
    beta, gamma, _ = node_rates(kind, n, seeds)
    both = sir_trajectories(g, seeds, beta, gamma, sims, T, rng_seed=21, edge_scan=scan)
    ev = sir_trajectories(g, seeds, beta, gamma, sims, T, rng_seed=21, edge_scan=scan, curves=False)
    cv = sir_trajectories(g, seeds, beta, gamma, sims, T, rng_seed=21, edge_scan=scan, events=False)
    assert ev.curves is None and cv.t_inf is None and cv.t_rec is None
    assert torch.equal(ev.t_inf, both.t_inf) and torch.equal(ev.t_rec, both.t_rec) and torch.equal(cv.curves, both.curves)


# -------------------------------------------------------------------------------------------------- 5. sharding
def test_shard_equals_slice_of_whole(dev):
    import torch
    from gnode.ode_nn import sir_trajectories
    kind, n, m, seeds, _, _ = SHAPE["er-small"]
    rp, ci, g = graph(kind, n, m)
    beta, gamma, _ = node_rates(kind, n, seeds)
    whole = sir_trajectories(g, seeds, beta, gamma, 1000, 12, rng_seed=5)
    part = sir_trajectories(g, seeds, beta, gamma, 40, 12, rng_seed=5, sim_offset=600)
    assert (whole.t_rec[600:640] >= 0).any()
    for a, b in zip(whole, part):
        assert torch.equal(a[600:640], b)


# -------------------------------------------------------------------------------------------------- 6. sims > workgroups
def test_more_trajectories_than_workgroups_lds(dev):
    """5 000 trajectories: every workgroup of the LDS forms takes several, one after the other."""
    from gnode.ode_nn import sir_trajectories
    c, want = case("nodes/many"), _want("nodes/many")
    g, seeds, beta, gamma, sims, T = graph("er300", 300, 600)[2], c.start, c.beta, c.gamma, c.sims, c.T
    live_events(c, expected("nodes/many"))
    for scan in (False, True):
        _same(_np(sir_trajectories(g, seeds, beta, gamma, sims, T, rng_seed=13, edge_scan=scan)), want, f"edge_scan={scan}")


def test_more_trajectories_than_workgroups_workspace_lists(dev):
    """1 100 trajectories on the workspace-list form, whose grid is capped at 1 024 (the CPU model is too slow here: the
    identities with the production call, and frontier == scan)."""
    import torch
    kind, n, m, seeds, _, _ = SHAPE["global-lists"]
    rp, ci, g = graph(kind, n, m)
    beta, gamma, _ = node_rates(kind, n, seeds)
    a = _check_identities(g, seeds, beta, gamma, 1100, 6, 17, "global-lists x 1100")
    b = _check_identities(g, seeds, beta, gamma, 1100, 6, 17, "global-lists x 1100, scan", edge_scan=True)
    assert (a.t_inf[1024:] > 0).any() and (a.t_rec[1024:] > 0).any()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# -------------------------------------------------------------------------------------------------- 7. large state
def test_large_state_paths(dev):
    """n = 100 000: the scan kernel keeps the trajectory state in memory, the frontier walk its lists (int32 ids)."""
    from gnode.ode_nn import sir_trajectories
    c, want = case("nodes/large"), _want("nodes/large")
    g, seeds, beta, gamma = graph("large", c.n, c.m)[2], c.start, c.beta, c.gamma
    live_events(c, expected("nodes/large"))
    for scan in (False, True):
        _same(_np(sir_trajectories(g, seeds, beta, gamma, 24, 8, rng_seed=99, edge_scan=scan)), want, f"large, edge_scan={scan}")


# -------------------------------------------------------------------------------------------------- 8. extinction, tail fill
def test_early_extinction_fills_the_tail(dev):
    from gnode.ode_nn import sir_trajectories
    kind, n, m, seeds, sims, T = SHAPE["isolated"]
    rp, ci, g = graph(kind, n, m)
    beta, gamma, _ = node_rates(kind, n, seeds)
    want = _want("nodes/isolated-1")
    cv = want[2].astype(np.int64)
    dead = cv[:, :, 1] == 0
    assert dead[:, :T - 2].any(), "no trajectory of the model is extinct before T - 2"
    assert not dead[:, T - 1].all(), "every trajectory of the model is extinct"
    for s in np.flatnonzero(dead.any(axis=1)):                       # the model's rows after extinction repeat the final state
        t0 = int(np.argmax(dead[s]))
        assert np.all(cv[s, t0:] == cv[s, t0])
    for scan in (False, True):
        _same(_np(sir_trajectories(g, seeds, beta, gamma, sims, T, rng_seed=21, edge_scan=scan)), want, f"isolated, edge_scan={scan}")


def test_certain_infection_follows_bfs_depth(dev):
    """beta = 1, gamma = 0: t_inf is the BFS depth on the seed's component, nobody recovers, and the epidemic stops."""
    from gnode.ode_nn import sir_trajectories
    n, seed, sims = 300, 11, 32
    rp, ci, g = graph("er300", n, 600)
    depth = bfs_depth(rp, ci, seed, n)
    ecc = int(depth.max())
    T = ecc + 2
    for scan in (False, True):
        t_inf, t_rec, curves = _np(sir_trajectories(g, [seed], np.ones(n), np.zeros(n), sims, T, rng_seed=3, edge_scan=scan))
        assert np.array_equal(t_inf, np.broadcast_to(depth.astype(np.int16), (sims, n)))
        assert np.all(t_rec == -1)
        within = np.array([(depth >= 0) & (depth <= t) for t in range(T)]).sum(axis=1)
        assert np.array_equal(curves[:, :, 1], np.broadcast_to(within.astype(np.uint32), (sims, T)))
        assert np.all(curves[:, :, 2] == 0) and np.array_equal(curves[:, :, 0], n - curves[:, :, 1])


# -------------------------------------------------------------------------------------------------- 9. everybody infected
def test_everybody_infected_branch(dev):
    """A connected graph, beta = 1, a seed that never recovers: everybody is infected by step ecc, and the remaining steps
    take the frontier kernel's recovery-only branch."""
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import sir_trajectories
    c, want = case("nodes/everybody"), _want("nodes/everybody")
    rp, ci, (seed,), beta, gamma, sims, T = c.rp, c.ci, c.start, c.beta, c.gamma, c.sims, c.T
    full = want[2][:, :, 0] == 0                                     # S_t = 0: n_ever == n
    assert full[:, T - 6].all(), "the model has not infected everybody 5 steps before the end"
    assert (want[1] >= T - 5).any(), "nobody recovers in the model's last five steps"
    g = DeviceGraph(rp, ci)
    for scan in (False, True):
        _same(_np(sir_trajectories(g, [seed], beta, gamma, sims, T, rng_seed=4, edge_scan=scan)), want, f"edge_scan={scan}")


# -------------------------------------------------------------------------------------------------- 10. bounds of the writes
@pytest.mark.parametrize("case", ["er-small", "odd-n-3-sims", "global-lists"])
@pytest.mark.parametrize("scan", [False, True], ids=["frontier", "scan"])
def test_writes_stay_inside_the_outputs(case, scan, dev):
    """The outputs are views into larger tensors filled with 0x5A5A...: the guards around them survive, nothing inside."""
    import gnode_oracle as O
    import torch
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import _sir_launch
    if case == "odd-n-3-sims":
        n, seeds, sims, T = 301, [4, 300], 3, 7
        rp, ci, _ = O.er_graph(n, 900, seed=301)
        g = DeviceGraph(rp, ci)
    else:
        _, n, m, seeds, sims, T = SHAPE[case]
        rp, ci, g = graph(case, n, m)
    rng = np.random.default_rng(55)
    beta, gamma = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
    ge, gc = 3, 5                                                     # guards; 3 int16: the view is 2-byte aligned only
    ne, nc = 2 * sims * n, sims * T * 3
    ebuf = torch.full((ge + ne + 2 * ge,), 0x5A5A, dtype=torch.int16, device=dev)
    cbuf = torch.full((gc + nc + gc,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ev, cv = ebuf[ge:ge + ne].view(2, sims, n), cbuf[gc:gc + nc].view(sims, T, 3)
    _sir_launch(g, seeds, beta, gamma, sims, T, 21, 0, ev, cv, None, scan)
    torch.cuda.synchronize()
    assert bool((ebuf[:ge] == 0x5A5A).all()) and bool((ebuf[ge + ne:] == 0x5A5A).all()), "events: a guard was written"
    assert bool((cbuf[:gc] == 0x5A5A5A5A).all()) and bool((cbuf[gc + nc:] == 0x5A5A5A5A).all()), "curves: a guard was written"
    assert not bool((ev == 0x5A5A).any()), "events: an element was not written"
    assert not bool((cv == 0x5A5A5A5A).any()), "curves: an element was not written"
    assert bool(((ev >= -1) & (ev < T)).all()) and bool((cv.sum(dim=2) == n).all())
    assert bool((ev[0] > 0).any())


# -------------------------------------------------------------------------------------------------- 11. sir_state_at
def test_sir_state_at(dev):
    import torch
    from gnode.ode_nn import sir_state_at, sir_trajectories
    kind, n, m, seeds, sims, T = SHAPE["er-small"]
    rp, ci, g = graph(kind, n, m)
    beta, gamma, _ = node_rates(kind, n, seeds)
    want = _want(f"nodes/{kind}")
    tr = sir_trajectories(g, seeds, beta, gamma, sims, T, rng_seed=21)
    for t in (0, T // 2, T - 1):
        st = sir_state_at(tr.t_inf, tr.t_rec, t)
        assert st.dtype == torch.int8 and st.shape == (sims, n) and st.device == tr.t_inf.device
        got = st.cpu().numpy()
        assert np.array_equal(got, states_at(want[0], want[1], t))
        # and, from the model's curves (counted from its state vectors, not from its events): the totals of each state
        totals = np.stack([(got == k).sum(axis=1) for k in range(3)], axis=1)
        assert np.array_equal(totals, want[2][:, t].astype(np.int64))
    assert (sir_state_at(tr.t_inf, tr.t_rec, T - 1) == 2).any()


# -------------------------------------------------------------------------------------------------- 12. sims = 0
def test_no_trajectories(dev):
    import torch
    from gnode import _lib
    from gnode.ode_nn import sir_counts_from_events, sir_curves_from_events, sir_trajectories
    kind, n, m, seeds, _, T = SHAPE["er-small"]
    rp, ci, g = graph(kind, n, m)
    tr = sir_trajectories(g, seeds, 0.3, 0.2, 0, T, rng_seed=1)
    assert tr.t_inf.shape == (0, n) and tr.t_rec.shape == (0, n) and tr.curves.shape == (0, T, 3)
    assert tr.t_inf.dtype == torch.int16 and tr.curves.dtype == torch.int32 and tr.t_inf.is_cuda
    assert sir_curves_from_events(tr.t_inf, tr.t_rec, T).shape == (0, T, 3)
    assert sir_counts_from_events(tr.t_inf, tr.t_rec, T).shape == (3, T, n)
    # the entry itself: sims == 0 is valid and touches neither output
    lib = _lib.load()
    ev = torch.full((2, 1, n), 0x5A5A, dtype=torch.int16, device=dev)
    cv = torch.full((1, T, 3), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.gnode_sir_traj_workspace_bytes(g.handle, T), dtype=torch.uint8, device=dev)
    sd = np.asarray(seeds, dtype=np.int32)
    import ctypes as C
    _lib.check(lib.gnode_sir_mc_philox_traj(g.handle, _lib.host_ptr(sd), 2, 0.3, 0.2, None, None, 0, 0, T, C.c_uint64(1),
                                            _lib.ptr(ev), _lib.ptr(cv), None, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(), 0))
    torch.cuda.synchronize()
    assert bool((ev == 0x5A5A).all()) and bool((cv == 0x5A5A5A5A).all())
    # argument errors of the entry: no output, one rate array, T past int16 with events
    rates = np.full(n, 0.3)
    for args in ((None, None, None, None, T), (rates, None, ev, cv, T), (None, None, ev, None, 40000)):
        b, gm, e_, c_, T_ = args
        status = lib.gnode_sir_mc_philox_traj(g.handle, _lib.host_ptr(sd), 2, 0.3, 0.2, _lib.host_ptr(b) if b is not None else None,
                                              _lib.host_ptr(gm) if gm is not None else None, 1, 0, T_, C.c_uint64(1),
                                              _lib.ptr(e_), _lib.ptr(c_), None, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(), 0)
        assert status == -1, (status, lib.gnode_last_error())          # GNODE_ERR_ARG
