"""GPU: the Monte-Carlo nowcast from evidence that may be wrong (gnode_sir_mc_philox_sweep_posterior_strata through
gnode.ode_nn.posterior_strata_mc) against tests/sir_strata_model.py, by INTEGER EQUALITY of the counts and the acceptances per
stratum, on the cases of tests/sir_post_model.py -- lists in LDS, rows past GN_SIR_BIGROW, lists in the workspace, the scan with
its state in LDS and in memory, the everybody-infected branch -- with eight evidence sets each at M = 2, and on the `lonely`
runs, whose trajectories end before `now`, between `now` and the last horizon, and never.  Then the identities on the device
with the same seed: stratum 0 is posterior_states_mc, accepted is source_scores_timed_mc's histogram read from the top, a
smaller M is a prefix, a never-matched record moves every stratum by one, and the stratum that holds everything has
outbreak_sizes_mc's sums; across shards, set groups and candidate lists, against an exact forward filter with a mismatch counter
on a graph with a loop, and through the entry's refusals.  tests/test_sir_strata_model.py runs the cases' liveness checks and
the chain on the CPU."""
import numpy as np
import pytest

import sir_cases as SC
import sir_post_model as PM
import sir_score_model as Q
import sir_strata_model as XM
import sir_timed_model as TM
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


def _host(r):
    return r.counts.cpu().numpy().astype(np.uint64), r.accepted.cpu().numpy().astype(np.uint64)


def _run(c, sets, shifts, dev, M=XM.M_CASES, cands=None, sims=None, one=False, **kw):
    """(counts uint64 [O, D, H, 2, n], accepted uint64 [O, C, D]) of a case through posterior_strata_mc, as host arrays; one:
    `sets` is one set of records, given as one object"""
    from gnode.ode_nn import posterior_strata_mc
    g = _graph(c)
    beta, gamma = _schedules(c, g)
    sims = c.sims if sims is None else sims
    now, horizons = XM.now_of(c.T), XM.horizons_of(c.T)
    obs = TM.Observations(c.n, sets) if one else [TM.Observations(c.n, s) for s in sets]
    cands = c.cands if cands is None else cands
    r = posterior_strata_mc(g, obs, beta, gamma, sims, c.T, now, horizons, M, candidates=cands, start=SC.state(c.p), shifts=shifts, rng_seed=c.rng_seed,
                            device=dev, **kw)
    O = 1 if one else len(sets)
    assert r.counts.dtype.is_floating_point is False and tuple(r.counts.shape) == (O, M + 1, len(horizons), 2, c.n) and tuple(r.accepted.shape) == (O, len(cands), M + 1)
    assert (r.sims, r.now, r.horizons, r.squeezed) == (sims, now, tuple(horizons), one)
    assert r.records == ((len(sets),) if one else tuple(len(s) for s in sets))
    return _host(r)


PATHS = [(*r, False) for r in XM.RUNS] + [(k, "mixed", True) for k in ("er-small/init", "large/init", "everybody")]


@pytest.mark.parametrize("key,shifts,edge_scan", PATHS)
def test_strata_equal_the_model_on_every_path(key, shifts, edge_scan, dev):
    c = XM.case(key)
    kind = c.base.shape[0] if c.base.shape else key
    if kind == "hubs":
        assert int(np.max(np.diff(c.rp))) > 512                    # rows past GN_SIR_BIGROW
    if kind == "global-lists":
        assert c.n > 11232                                         # the lists do not fit LDS
    if kind == "large":
        assert 2 * c.n > 150 * 1024                                # the scan's state does not fit LDS
    counts, accepted = _run(c, XM.sets_of(key, shifts), getattr(c, shifts), dev, edge_scan=edge_scan)
    want_counts, want_accepted = XM.expected(key, shifts)
    assert np.array_equal(accepted, want_accepted)
    assert np.array_equal(counts, want_counts)


@pytest.mark.parametrize("key,edge_scan", [(k, False) for k in XM.KEYS] + [("er-small/init", True), ("large/init", True)])
def test_lonely_runs_equal_the_model(key, edge_scan, dev):
    """trajectories that end before `now`, between `now` and the last horizon, and never: the final state stays in its stratum"""
    from gnode.ode_nn import posterior_strata_mc
    r = PM.lonely(key)
    c = XM.case(key)
    got = posterior_strata_mc(_graph(c), [TM.Observations(r.n, s) for s in XM.lonely_sets(key)], 0.0, r.gamma, r.sims, r.T, r.now, r.horizons, XM.M_LONELY,
                              candidates=r.cands, rng_seed=r.rng_seed, edge_scan=edge_scan, device=dev)
    counts, accepted = _host(got)
    want_counts, want_accepted = XM.lonely_expected(key)
    assert np.array_equal(accepted, want_accepted) and np.array_equal(counts, want_counts)


@pytest.mark.parametrize("key", ["er-small/init", "everybody"])
def test_the_identities_on_the_device(key, dev):
    """with the same seed: stratum 0 is posterior_states_mc's two tensors; accepted[o, c, d] is what source_scores_timed_mc of set
    o alone counts at age `now` in bin R_o - d (bins = R_o by default); M = 0 and M = 1 give the first strata of M = 2; (d1) is
    (d) moved by one stratum; stratum 2 of (e2) holds every trajectory, and its counts summed over the nodes are
    outbreak_sizes_mc's sums summed over the candidates"""
    from gnode.ode_nn import outbreak_sizes_mc, posterior_states_mc, source_scores_timed_mc
    c = XM.case(key)
    g = _graph(c)
    beta, gamma = _schedules(c, g)
    sets = XM.sets_of(key, "mixed")
    now, hz = XM.now_of(c.T), XM.horizons_of(c.T)
    common = dict(candidates=c.cands, start=SC.state(c.p), shifts=c.mixed, rng_seed=c.rng_seed, device=dev)
    counts, accepted = _run(c, sets, c.mixed, dev)
    post = posterior_states_mc(g, [TM.Observations(c.n, s) for s in sets], beta, gamma, c.sims, c.T, now, hz, **common)
    post_counts, post_accepted = _host(post)
    assert np.array_equal(counts[:, 0], post_counts) and np.array_equal(accepted[..., 0], post_accepted)
    for o, s in enumerate(sets):
        t = source_scores_timed_mc(g, TM.Observations(c.n, s), beta, gamma, c.sims, c.T, **common)
        assert t.bins == len(s)
        hist = t.hist[0, :, now].cpu().numpy().astype(np.uint64)    # [C, R_o + 1]
        for d in range(min(len(s), XM.M_CASES) + 1):
            assert np.array_equal(accepted[o, :, d], hist[:, len(s) - d]), (o, d)
        assert (accepted[o, :, len(s) + 1:] == 0).all()             # nobody misses more records than there are
    for M in (0, 1):
        less = _run(c, sets, c.mixed, dev, M=M)
        assert np.array_equal(less[0], counts[:, :M + 1]) and np.array_equal(less[1], accepted[..., :M + 1]), M
    assert np.array_equal(accepted[XM.D1, :, 1:], accepted[XM.D, :, :2]) and np.array_equal(counts[XM.D1, 1:], counts[XM.D, :2])
    assert (accepted[XM.D1, :, 0] == 0).all() and (counts[XM.D1, 0] == 0).all() and accepted[XM.D, :, 0].sum() > 0
    assert (accepted[XM.E2, :, 2] == c.sims).all() and (accepted[XM.E2, :, :2] == 0).all() and (accepted[XM.E3] == 0).all() and (counts[XM.E3] == 0).all()
    s = outbreak_sizes_mc(g, beta, gamma, c.sims, c.T, candidates=c.cands, start=SC.state(c.p), shifts=c.mixed, rng_seed=c.rng_seed, device=dev)
    sums = s.sums.cpu().numpy().astype(np.uint64)
    for j, h in enumerate(hz):
        assert np.array_equal(counts[XM.E2, 2, j].sum(-1), sums[:, now + h, 1:3].sum(0)), (key, h)


def test_two_shards_of_the_sims_range_accumulate_to_the_whole(dev):
    import torch
    c = XM.case("er-small/init")
    sets = XM.sets_of("er-small/init", "mixed")
    want_counts, want_accepted = XM.expected("er-small/init", "mixed")
    cut = 13
    counts = torch.zeros((8, 3, 3, 2, c.n), dtype=torch.int64, device=dev)
    accepted = torch.zeros((8, len(c.cands), 3), dtype=torch.int64, device=dev)
    a = _run(c, sets, c.mixed, dev, sims=cut, sim_offset=0, counts=counts, accepted=accepted)
    assert not np.array_equal(a[0], want_counts) and (a[1][XM.E2, :, 2] == cut).all()
    b = _run(c, sets, c.mixed, dev, sims=c.sims - cut, sim_offset=cut, counts=counts, accepted=accepted)
    assert np.array_equal(b[0], want_counts) and np.array_equal(b[1], want_accepted)
    rest = _run(c, sets, c.mixed, dev, sims=c.sims - cut, sim_offset=cut)
    assert np.array_equal(rest[0], want_counts - a[0]) and np.array_equal(rest[1], want_accepted - a[1])


def _many_sets(key, shifts, count, seed):
    """`count` evidence sets: the case's (a), (d), (d1), (e2), thinned at random, rotated; the last one is none of the others"""
    base = [XM.sets_of(key, shifts)[i] for i in (XM.A, XM.D, XM.D1, XM.E2)]
    rng = np.random.default_rng(seed)
    sets = []
    for i in range(count):
        s = [r for r in base[i % 4] if rng.random() >= 0.1 * (i % 5)] or [base[i % 4][0]]
        sets.append(s)
    sets[-1] = [base[0][0], base[0][-1]]
    return sets


def test_seventeen_sets_are_two_groups_and_equal_seventeen_calls(dev):
    c = XM.case("er-small/init")
    sets = _many_sets("er-small/init", "zeros", 17, 17)
    counts, accepted = _run(c, sets, c.zeros, dev)
    for o in range(17):
        one = _run(c, sets[o], c.zeros, dev, one=True)
        assert np.array_equal(counts[o], one[0][0]) and np.array_equal(accepted[o], one[1][0]), o
    assert accepted[16].sum() == c.sims * len(c.cands) and not np.array_equal(counts[16], counts[0])      # two records: complete at M = 2
    assert (accepted[:, :, 1].sum(1) > 0).any() and (accepted[:, :, 2].sum(1) > 0).any()


def test_candidate_lists_with_repeats_and_other_orders(dev):
    """accepted[:, c] does not depend on the list; the counts add over the list, a repeated candidate counting twice"""
    c = XM.case("er-small/init")
    sets = XM.sets_of("er-small/init", "mixed")
    ev = XM.case_events("er-small/init", "mixed")
    now, hz = XM.now_of(c.T), XM.horizons_of(c.T)
    for pick in ([4, 2], [3, 0, 1, 2, 2, 4, 2], list(range(len(c.cands)))[::-1]):
        want_counts, want_accepted = XM.strata_of([ev[j] for j in pick], sets, c.T, now, hz, c.n, XM.M_CASES)
        cnt, acc = _run(c, sets, [c.mixed[j] for j in pick], dev, cands=[c.cands[j] for j in pick])
        assert np.array_equal(acc, want_accepted) and np.array_equal(cnt, want_counts), pick
    many = list(range(0, c.n, 7)) + [-1]                            # more candidates than workgroups' worth of one: 73 x 3 jobs
    cnt, acc = _run(c, sets, None, dev, cands=many, sims=3)
    one = _run(c, sets, None, dev, cands=[many[11]], sims=3)
    assert np.array_equal(acc[:, 11], one[1][:, 0]) and (acc[XM.E2, :, 2] == 3).all()


def test_one_object_the_methods_and_no_trajectories(dev):
    """one object drops the set axis in the methods, which read the device's integers; sims = 0 touches nothing"""
    import torch
    from gnode.ode_nn import posterior_strata_mc
    c = XM.case("er-small/init")
    g = _graph(c)
    beta, gamma = _schedules(c, g)
    records = XM.sets_of("er-small/init", "zeros")[XM.D]
    want_counts, want_accepted = XM.expected("er-small/init", "zeros")
    now, hz = XM.now_of(c.T), XM.horizons_of(c.T)
    r = posterior_strata_mc(g, TM.Observations(c.n, records), beta, gamma, c.sims, c.T, now, hz, 2, candidates=c.cands, start=SC.state(c.p), shifts=c.zeros,
                            rng_seed=c.rng_seed, device=dev)
    by = want_accepted[XM.D].sum(0).astype(np.float64)              # [140, 60, 0]
    assert r.squeezed and r.records == (2,) and bool(r.complete()) and r.by_stratum().tolist() == by.tolist()
    w = np.asarray([1.0, 0.05 / 0.95, (0.05 / 0.95) ** 2])
    m = r.marginals(error=0.05).cpu().numpy()
    assert m.shape == (3, c.n, 3) and np.allclose(m[..., 1], (want_counts[XM.D][:, :, 0] * w[:, None, None]).sum(0) / (by * w).sum(), rtol=1e-13, atol=0)
    assert np.allclose(m.sum(-1), 1.0, rtol=0, atol=1e-14)
    assert np.isclose(float(r.ess(error=0.05)), (by * w).sum() ** 2 / (by * w * w).sum(), rtol=1e-13) and float(r.ess(error=0.05)) > float(r.ess(error=0)) == by[0]
    assert np.allclose(r.source(weights=[1, 1, 1]).cpu().numpy(), 1.0 / len(c.cands), rtol=1e-15)          # complete and flat: nothing is learnt
    assert torch.equal(r.exact().counts, r.counts[:, 0]) and int(r.exact().accepted_total()) == int(by[0])
    counts = torch.full((1, 3, 3, 2, c.n), 7, dtype=torch.int64, device=dev)
    accepted = torch.full((1, len(c.cands), 3), 7, dtype=torch.int64, device=dev)
    z = posterior_strata_mc(g, TM.Observations(c.n, records), beta, gamma, 0, c.T, now, hz, 2, candidates=c.cands, start=SC.state(c.p), shifts=c.zeros,
                            rng_seed=c.rng_seed, counts=counts, accepted=accepted, device=dev)
    assert bool((z.counts == 7).all()) and bool((z.accepted == 7).all()) and z.sims == 0


@pytest.mark.parametrize("edge_scan", [False, True])
def test_the_exact_chain_on_a_graph_with_a_loop(edge_scan, dev):
    """The triangle with a pendant node of tests/test_sir_strata_model.py, T = 8, sims = 20 000, (set, now) = (D, 1), (F, 3), (G, 2),
    (D, 0), (F, 4), horizons (0, 1, 3), M = 3 (every set complete), ONE CALL PER CANDIDATE (the candidates share their coins):
    integer-equal to the model, which tests/test_sir_strata_model.py holds against the exact filter with a mismatch counter --
    every cell of counts / sims and accepted / sims within 5 sqrt(P (1 - P) / sims) + 1 / sims, zero where the filter is zero --
    and held against it here again.  On the model the largest share of the bound is 0.683 and 1 060 cells have P >= 0.01."""
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import posterior_strata_mc
    rp, ci = Q.chain_csr()
    g = DeviceGraph(rp, ci)
    worst, cells = 0.0, 0
    for name, now in XM.CHAIN_RUNS:
        obs = TM.Observations(Q.CHAIN_N, TM.CHAIN_SETS[name])
        per = [_host(posterior_strata_mc(g, obs, Q.CHAIN_W, Q.CHAIN_GAMMA, XM.CHAIN_SIMS, TM.CHAIN_T, now, XM.CHAIN_HORIZONS, XM.CHAIN_M, candidates=[cand],
                                         rng_seed=Q.CHAIN_RNG, edge_scan=edge_scan, device=dev)) for cand in range(Q.CHAIN_N)]
        counts, accepted = np.stack([c[0] for c, _ in per]), np.stack([a[0, 0] for _, a in per])
        want_counts, want_accepted = XM.chain_counts(name, now)
        assert np.array_equal(counts, want_counts) and np.array_equal(accepted, want_accepted)
        share, k = XM.check_chain(name, now, counts, accepted)
        worst, cells = max(worst, share), cells + k
    print("largest share of the bound", worst, "cells with P >= 0.01", cells)
    assert worst <= 1.0 and cells == 1060


def test_the_entry_refuses_and_writes_nothing(dev):
    """through the C entry: mismatches -1 and 8, what the posterior entry refuses (O, now, H, the horizons, the records, the
    sweep's arguments, null outputs), a short workspace; both outputs keep their fill, and a good call after them is served"""
    import ctypes as C
    import torch
    from gnode import _lib
    c = XM.case("er-small/init")
    g = _graph(c)
    lib = _lib.load()
    ARG, WORKSPACE = -1, -3
    n, T, P, L, Cn, sims, M = c.n, c.T, c.P, c.L, len(c.cands), 4, XM.M_CASES
    now, hz = XM.now_of(T), np.asarray(XM.horizons_of(T), np.int32)
    W, Gm = np.ascontiguousarray(np.stack(c.W)), np.ascontiguousarray(np.stack([np.broadcast_to(x, (n,)) for x in c.G]).astype(np.float64))
    init, phase = np.ascontiguousarray(c.p), np.ascontiguousarray(c.phase)
    cand, shifts = np.asarray(c.cands, np.int32), np.asarray(c.mixed, np.int32)
    sets = XM.sets_of("er-small/init", "mixed")
    rec = np.ascontiguousarray([(o, *r) for o, s in enumerate(sets) for r in s], np.int32)      # [R, 4]: set, node, offset, kind
    R, O, H = len(rec), len(sets), len(hz)
    need = lib.gnode_sir_sweep_posterior_workspace_bytes(g.handle, T, P, L, Cn, O, R, H)        # the posterior's: D sizes only the outputs
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.full((O, M + 1, H, 2, n), 7, dtype=torch.int64, device=dev)
    accepted = torch.full((O, Cn, M + 1), 7, dtype=torch.int64, device=dev)

    def call(init=init, cand=cand, shifts=shifts, Cn=Cn, action=0, phase=phase, P=P, L=L, W=W, Gm=Gm, rec=rec, R=R, O=O, now=now, hz=hz, H=H, M=M, sims=sims,
             T=T, nbytes=need, out=counts, acc=accepted):
        hp = lambda a: None if a is None else _lib.host_ptr(a)      # noqa: E731
        cols = [None] * 4 if rec is None else [np.ascontiguousarray(rec[:, j]) for j in range(4)]
        hz32 = None if hz is None else np.ascontiguousarray(hz, np.int32)
        return lib.gnode_sir_mc_philox_sweep_posterior_strata(g.handle, hp(init), hp(cand), hp(shifts), Cn, action, hp(phase), P, L, hp(W), hp(Gm),
                                                              *(hp(x) for x in cols), R, O, now, hp(hz32), H, M, sims, 0, T, C.c_uint64(c.rng_seed),
                                                              _lib.ptr(out), _lib.ptr(acc), _lib.ptr(ws), nbytes, _lib.stream_ptr(), 0)

    def changed(i, j, value):
        x = rec.copy(); x[i, j] = value
        return x

    said = lambda: lib.gnode_last_error().decode()                  # noqa: E731
    assert call(M=-1) == ARG and "mismatches = -1" in said() and "gnode_sir_mc_philox_sweep_posterior_strata" in said()
    assert call(M=8) == ARG and "mismatches = 8" in said()
    assert call(O=0) == ARG and "O = 0" in said()
    assert call(O=17) == ARG and "O = 17" in said()
    assert call(now=-1) == ARG and "now = -1" in said()
    assert call(now=T) == ARG and f"now = {T}" in said()
    assert call(H=0) == ARG and "H = 0" in said()
    assert call(H=33) == ARG and "H = 33" in said()
    assert call(hz=[-1, 0, 1]) == ARG and "horizons[0] = -1" in said()
    assert call(hz=[0, 1, 1]) == ARG and "horizons[2] = 1" in said()
    assert call(hz=[0, 1, T - now]) == ARG and f"horizons[2] = {T - now}" in said()
    assert call(hz=None) == ARG and call(R=0) == ARG and "R = 0" in said()
    assert call(rec=changed(7, 0, O)) == ARG and f"rec_set[7] = {O}" in said()
    assert call(rec=changed(9, 1, n)) == ARG and f"rec_node[9] = {n}" in said()
    assert call(rec=changed(2, 3, 5)) == ARG and "rec_kind[2] = 5" in said()
    assert call(rec=changed(R - 1, 2, 1)) == ARG and f"rec_offset[{R - 1}] = 1" in said()
    assert call(rec=rec[rec[:, 0] != 1], R=int((rec[:, 0] != 1).sum())) == ARG and "evidence set 1 holds no record" in said()
    assert call(rec=None) == ARG and call(out=None) == ARG and call(acc=None) == ARG and call(init=None) == ARG
    x = shifts.copy(); x[3] = L - T + 1
    assert call(shifts=x) == ARG and f"shifts[3] = {L - T + 1}" in said()
    assert call(Cn=0) == ARG and call(action=2) == ARG and call(L=T - 1) == ARG and call(P=0) == ARG and call(sims=-1) == ARG and call(T=0) == ARG
    assert call(nbytes=need - 1) == WORKSPACE
    assert call(sims=0) == 0, said()                                # valid, and touches nothing
    torch.cuda.synchronize()
    assert bool((counts == 7).all()) and bool((accepted == 7).all())
    counts.zero_(); accepted.zero_()
    assert call() == 0, said()
    want_counts, want_accepted = XM.expected("er-small/init", "mixed", sims=sims)
    assert np.array_equal(counts.cpu().numpy().astype(np.uint64), want_counts) and np.array_equal(accepted.cpu().numpy().astype(np.uint64), want_accepted)
