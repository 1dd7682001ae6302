"""GPU: Monte-Carlo outbreak sizes for many candidates in one launch (gnode_sir_mc_philox_sweep through
gnode.ode_nn.outbreak_sizes_mc) against tests/sir_sweep_model.py, by INTEGER EQUALITY of the sums and of the per-trajectory
sizes, on the shapes of tests/schedule_cases.py -- lists in LDS, rows past GN_SIR_BIGROW, lists in the workspace, the scan
with its state in LDS and in memory, the everybody-infected branch -- with four to six candidates each (no change, a node the
start already infects, the hub twice, the last node, a node of degree 0), both actions, no shifts and shifts that reach the
last entry of a phase row longer than T.  C * sims stays at or below the shape's own sims.  Then against the parent's code (one
sir_trajectories call per candidate), across shards, across candidate lists, through the identity between `ever` and the
sums, through the entry's refusals, and against DMP on a tree.  tests/test_sir_sweep_host.py runs the cases' liveness checks
on the CPU."""
import numpy as np
import pytest

import schedule_cases as K
import sir_cases as SC
import sir_sweep_model as S
from sir_cases import dev  # noqa: F401

pytestmark = pytest.mark.gpu


def _graph(c):
    if c.base.shape is not None:
        return SC.graph(*c.base.shape)[2]
    from gnode.graph import DeviceGraph
    return DeviceGraph(c.rp, c.ci)


def _schedules(c, g, phase=None):
    from gnode.ode_nn import rate_schedule
    phase = c.phase if phase is None else phase
    return rate_schedule([SC.er_of(g, w) for w in c.W], steps=phase), rate_schedule(list(c.G), steps=phase)


def _run(c, action, shifts, dev, cands=None, sims=None, **kw):
    """(sums uint64 [C, T, 3], ever uint32 [C, sims]) of a case through outbreak_sizes_mc, as host arrays"""
    from gnode.ode_nn import outbreak_sizes_mc
    g = _graph(c)
    beta, gamma = _schedules(c, g)
    r = outbreak_sizes_mc(g, beta, gamma, c.sims if sims is None else sims, c.T, candidates=c.cands if cands is None else cands, action=action,
                          start=SC.state(c.p), shifts=shifts, rng_seed=c.rng_seed, per_trajectory=True, device=dev, **kw)
    assert r.sums.dtype.is_floating_point is False and tuple(r.sums.shape) == (len(c.cands if cands is None else cands), c.T, 3)
    return r.sums.cpu().numpy().astype(np.uint64), SC.u32(r.ever)


def _same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[1].sum(1, dtype=np.int64), S.infections(got[0]))     # sum_s ever = infections(sums)


PATHS = [(k, a, s, False) for k, a, s in S.RUNS] + [(k, a, s, True) for k, a, s in S.RUNS if k in ("er-small/init", "large/init", "everybody")]


@pytest.mark.parametrize("key,action,shifts,edge_scan", PATHS)
def test_sums_and_ever_equal_the_model_on_every_path(key, action, shifts, edge_scan, dev):
    c = S.case(key)
    kind = c.base.shape[0] if c.base.shape else key
    if kind == "hubs":
        assert int(np.max(np.diff(c.rp))) > 512                    # rows past GN_SIR_BIGROW
    if kind == "global-lists":
        assert c.n > 11232                                         # the lists do not fit LDS
    if kind == "large":
        assert 2 * c.n > 150 * 1024                                # the scan's state does not fit LDS
    _same(_run(c, action, getattr(c, shifts), dev, edge_scan=edge_scan), S.expected(key, action, shifts))


@pytest.mark.parametrize("action,shifts", [("seed", "mixed"), ("immunise", "mixed")])
def test_er_small_equals_one_call_of_the_parents_code_per_candidate(action, shifts, dev):
    """curves.sum(0) of gnode_sir_mc_philox_schedule from the start with the candidate's row replaced, under the phase row
    moved by the candidate's shift"""
    from gnode.ode_nn import sir_trajectories
    c = S.case("er-small/init")
    g = _graph(c)
    sums, ever = _run(c, action, getattr(c, shifts), dev)
    for j, (cand, k) in enumerate(zip(c.cands, getattr(c, shifts))):
        p = np.array(c.p)
        if cand >= 0:
            p[cand] = S.ROW[action]
        beta, gamma = _schedules(c, g, c.phase[k:])
        r = sir_trajectories(g, SC.state(p), beta, gamma, c.sims, c.T, rng_seed=c.rng_seed, events=True, curves=True, device=dev)
        assert np.array_equal(r.curves.sum(0).cpu().numpy().astype(np.uint64), sums[j]), (j, cand, k)
        started_r = (r.t_rec == 0)
        assert np.array_equal(((r.t_inf >= 0) & ~started_r).sum(1).cpu().numpy().astype(np.uint32), ever[j])


def test_two_shards_of_the_sims_range_accumulate_to_the_whole(dev):
    import torch
    c = S.case("er-small/init")
    want = S.expected("er-small/init", "seed", "mixed")
    cut = 13
    sums = torch.zeros((len(c.cands), c.T, 3), dtype=torch.int64, device=dev)
    a = _run(c, "seed", c.mixed, dev, sims=cut, sim_offset=0, sums=sums)
    assert not np.array_equal(a[0], want[0])
    b = _run(c, "seed", c.mixed, dev, sims=c.sims - cut, sim_offset=cut, sums=sums)
    assert np.array_equal(b[0], want[0]) and np.array_equal(np.concatenate([a[1], b[1]], axis=1), want[1])
    off = _run(c, "seed", c.mixed, dev, sims=7, sim_offset=cut)     # the coins are those of sim_offset + s
    assert np.array_equal(off[1], want[1][:, cut:cut + 7])


def test_a_candidates_rows_do_not_depend_on_the_list(dev):
    """alone, at another position, next to other neighbours, in a list of other length: the same rows"""
    c = S.case("er-small/init")
    want = S.expected("er-small/init", "immunise", "mixed")
    for pick in ([2], [4, 2], [3, 0, 5 % len(c.cands), 1, 2, 2, 4], list(range(len(c.cands)))[::-1]):
        got = _run(c, "immunise", [c.mixed[j] for j in pick], dev, cands=[c.cands[j] for j in pick])
        assert np.array_equal(got[0], want[0][pick]) and np.array_equal(got[1], want[1][pick]), pick
    many = list(range(0, c.n, 7)) + [-1]                            # more candidates than workgroups' worth of one: 73 x 3 jobs
    got = _run(c, "seed", None, dev, cands=many, sims=3)
    one = _run(c, "seed", None, dev, cands=[many[11]], sims=3)
    assert np.array_equal(got[0][11], one[0][0]) and np.array_equal(got[1][11], one[1][0])
    assert np.array_equal(got[1].sum(1, dtype=np.int64), S.infections(got[0]))


def test_defaults_sizes_and_no_trajectories(dev):
    """candidates default to every node, `.sizes()` is sums / sims and `infections` reads it; sims = 0 touches nothing"""
    import torch
    from gnode.dmp import infections
    from gnode.ode_nn import outbreak_sizes_mc
    G, n, rp, ci = SC.karate()
    r = outbreak_sizes_mc(G, 0.2, 0.3, 50, 8, start=[0], rng_seed=3, per_trajectory=True, device=dev)
    assert tuple(r.sums.shape) == (n, 8, 3) and tuple(r.ever.shape) == (n, 50) and r.sims == 50 and r.sizes().dtype == torch.float64
    assert bool((r.sums.sum(2) == 50 * n).all())
    assert torch.equal(infections(r.sums), r.ever.sum(1).double())     # (infections reads the integer sums as well)
    assert torch.allclose(infections(r.sizes()), r.ever.double().mean(1), rtol=1e-12, atol=0) and torch.equal(r.sizes(), r.sums.double() / 50)
    want = S.sweep(n, rp, ci, np.asarray(SC.M.one_hot_init(n, [0])), list(range(n)), [0] * n, "seed", [np.full(len(ci), 0.2)], [0.3], np.zeros(8, int),
                   50, 8, 3)
    assert np.array_equal(r.sums.cpu().numpy().astype(np.uint64), want[0]) and np.array_equal(SC.u32(r.ever), want[1])
    sums = torch.full((n, 8, 3), 7, dtype=torch.int64, device=dev)
    z = outbreak_sizes_mc(G, 0.2, 0.3, 0, 8, start=[0], rng_seed=3, per_trajectory=True, sums=sums, device=dev)
    assert bool((z.sums == 7).all()) and tuple(z.ever.shape) == (n, 0)


def test_the_entry_refuses_and_writes_nothing(dev):
    """through the C entry: C < 1, an action other than 0 / 1, L < T, a bad shift, a phase out of range beyond T, what the
    scheduled entry refuses, a short workspace; sums and ever keep their fill, sims = 0 touches neither, and a good call after
    them is served"""
    import ctypes as C
    import torch
    from gnode import _lib
    c = S.case("er-small/init")
    g = _graph(c)
    lib = _lib.load()
    ARG, WORKSPACE = -1, -3
    n, nnz, T, P, L, Cn, sims = c.n, len(c.ci), c.T, c.P, c.L, len(c.cands), 4
    W, Gm = np.ascontiguousarray(np.stack(c.W)), np.ascontiguousarray(np.stack([np.broadcast_to(x, (n,)) for x in c.G]).astype(np.float64))
    init, phase = np.ascontiguousarray(c.p), np.ascontiguousarray(c.phase)
    cand, shifts = np.asarray(c.cands, np.int32), np.asarray(c.mixed, np.int32)
    need = lib.gnode_sir_sweep_workspace_bytes(g.handle, T, P, L, Cn)
    sched = lib.gnode_sir_schedule_workspace_bytes(g.handle, T, P)
    assert 0 < need <= sched - 2 * T * n * 4                        # smaller than the scheduled call's by the histogram at least
    for bad in ((None, T, P, L, Cn), (g.handle, 0, P, L, Cn), (g.handle, T, 0, L, Cn), (g.handle, T, P, T - 1, Cn), (g.handle, T, P, L, 0)):
        assert lib.gnode_sir_sweep_workspace_bytes(*bad) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    sums = torch.full((Cn, T, 3), 7, dtype=torch.int64, device=dev)
    ever = torch.full((Cn, sims), 7, dtype=torch.int32, device=dev)

    def call(init=init, cand=cand, shifts=shifts, Cn=Cn, action=0, phase=phase, P=P, L=L, W=W, Gm=Gm, sims=sims, T=T, nbytes=need, outs=(sums, ever)):
        hp = lambda a: None if a is None else _lib.host_ptr(a)      # noqa: E731
        return lib.gnode_sir_mc_philox_sweep(g.handle, hp(init), hp(cand), hp(shifts), Cn, action, hp(phase), P, L, hp(W), hp(Gm), sims, 0, T,
                                             C.c_uint64(c.rng_seed), *(_lib.ptr(o) for o in outs), _lib.ptr(ws), nbytes, _lib.stream_ptr(), 0)

    said = lambda: lib.gnode_last_error().decode()                  # noqa: E731
    assert call(Cn=0) == ARG and call(action=2) == ARG and call(action=-1) == ARG
    assert call(L=T - 1) == ARG and f"L = {T - 1}" in said()
    x = shifts.copy(); x[3] = L - T + 1
    assert call(shifts=x) == ARG and f"shifts[3] = {L - T + 1}" in said()
    x = shifts.copy(); x[1] = -1
    assert call(shifts=x) == ARG and "shifts[1] = -1" in said()
    x = phase.copy(); x[L - 1] = P
    assert call(phase=x) == ARG and f"phase[{L - 1}] = {P}" in said()
    assert call(phase=x, shifts=None) == ARG                        # ... whether or not a shift reaches it
    assert call(P=0) == ARG and call(init=None) == ARG and call(cand=None) == ARG and call(outs=(None, ever)) == ARG
    x = W.copy(); x[1, 17] = 1.25
    assert call(W=x) == ARG and "phase 1" in said() and "position 17" in said()
    x = init.copy(); x[5] = (0.5, 0.5, 0.5)
    assert call(init=x) == ARG and "node 5" in said()
    assert call(sims=-1) == ARG and call(T=0) == ARG
    assert call(nbytes=need - 1) == WORKSPACE
    assert call(sims=0) == 0, said()                                # valid, and touches neither output
    torch.cuda.synchronize()
    assert bool((sums == 7).all()) and bool((ever == 7).all())
    sums.zero_()
    x = phase.copy(); x[0] = 99                                     # entry 0 is never read
    assert call(phase=x) == 0, said()
    want = S.expected("er-small/init", "seed", "mixed", sims=sims)
    assert np.array_equal(sums.cpu().numpy().astype(np.uint64), want[0]) and np.array_equal(SC.u32(ever), want[1])
    sums.zero_()
    assert call(shifts=None, outs=(sums, None)) == 0, said()        # no shifts, no per-trajectory output
    assert np.array_equal(sums.cpu().numpy().astype(np.uint64), S.expected("er-small/init", "seed", "zeros", sims=sims)[0])
    assert bool((ever.cpu() == torch.from_numpy(want[1].astype(np.int32))).all())


def test_dmp_is_the_expectation_on_a_tree(dev):
    """The tree of sir_cases.tree_case() (120 nodes) under schedule_cases.tree()'s three-phase schedule, every node a candidate
    to seed, shifts 0 / 1 / 2 in rotation, T = 10: DMP is exact on a tree, so infections(outbreak_sizes_schedule(...)) and
    ever.mean(1) agree for every candidate within 5 std(ever[c]) / sqrt(sims) + 1 / sims -- the 5-sigma rule with the empirical
    deviation, a size not being a Bernoulli cell.  sims = 2000, rng seed 4321: verified on the CPU before any GPU run, the model
    alone (tests/sir_sweep_model.py tree_ever against tree_dmp) uses at most 0.351 of the bound over the 120 candidates (0.514
    and 0.179 under the seeds 99 and 7); tests/test_sir_sweep_host.py repeats it for every eighth node."""
    import scipy.sparse as sp
    import torch
    from gnode.dmp import infections, outbreak_sizes_schedule
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import outbreak_sizes_mc, rate_schedule
    n, rp, ci, W, G, p = K.tree()
    T, sims, cands = S.TREE_T, S.TREE_SIMS, list(range(n))
    shifts = S.tree_shifts(cands)
    steps = K.TREE_PHASE
    g = DeviceGraph(rp, ci)
    r = outbreak_sizes_mc(g, rate_schedule([SC.er_of(g, w) for w in W], steps=steps), rate_schedule(list(G), steps=steps), sims, T, candidates=cands,
                          action=S.TREE_ACTION, start=SC.state(p), shifts=shifts, rng_seed=S.TREE_RNG, per_trajectory=True, device=dev)
    mats = [sp.csr_matrix((np.asarray(w), np.asarray(ci), np.asarray(rp)), shape=(n, n)) for w in W]
    dmp = infections(outbreak_sizes_schedule(rate_schedule(mats, steps=steps), rate_schedule(list(G), steps=steps), T, candidates=cands,
                                             action=S.TREE_ACTION, start=SC.state(p), shifts=shifts, device=dev)).cpu().numpy()
    ever = SC.u32(r.ever)
    assert np.allclose(infections(r.sizes()).cpu().numpy(), ever.mean(1), rtol=1e-12, atol=0)
    ratio = S.tree_ratio(dmp, ever)
    print("largest share of the bound:", float(ratio.max()), "at candidate", int(ratio.argmax()))
    assert np.abs(dmp - S.tree_dmp(cands)).max() <= 1e-3            # the device's DMP is the model's, up to float32
    assert ratio.max() <= 1.0
