"""GPU: Monte-Carlo nowcast and forecast from timed evidence (gnode_sir_mc_philox_sweep_posterior through
gnode.ode_nn.posterior_states_mc) against tests/sir_post_model.py, by INTEGER EQUALITY of the counts and the acceptances, on the
cases of tests/sir_timed_model.py -- lists in LDS, rows past GN_SIR_BIGROW, lists in the workspace, the scan with its state in
LDS and in memory, the everybody-infected branch -- with five evidence sets each at now = T // 2 and three horizons, and on the
`lonely` runs, whose trajectories end before `now`, between `now` and the last horizon, and never.  Then against the existing
code (one sir_trajectories call per candidate, reduced in torch by the definition), against source_scores_timed_mc and
outbreak_sizes_mc where they must coincide, across shards, set groups and candidate lists, against an exact forward filter on a
graph with a loop, and through the entry's refusals.  tests/test_sir_post_model.py runs the cases' liveness checks and the chain
on the CPU."""
import numpy as np
import pytest

import sir_cases as SC
import sir_post_model as PM
import sir_score_model as Q
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


def _run(c, sets, shifts, dev, cands=None, sims=None, one=False, now=None, horizons=None, **kw):
    """(counts uint64 [O, H, 2, n], accepted uint64 [O, C]) of a case through posterior_states_mc, as host arrays; one: `sets` is
    one set of records, given as one object"""
    from gnode.ode_nn import posterior_states_mc
    g = _graph(c)
    beta, gamma = _schedules(c, g)
    sims = c.sims if sims is None else sims
    now, horizons = PM.now_of(c.T) if now is None else now, PM.horizons_of(c.T) if horizons is None else horizons
    obs = TM.Observations(c.n, sets) if one else [TM.Observations(c.n, s) for s in sets]
    cands = c.cands if cands is None else cands
    r = posterior_states_mc(g, obs, beta, gamma, sims, c.T, now, horizons, candidates=cands, start=SC.state(c.p), shifts=shifts, rng_seed=c.rng_seed,
                            device=dev, **kw)
    O = 1 if one else len(sets)
    assert r.counts.dtype.is_floating_point is False and tuple(r.counts.shape) == (O, len(horizons), 2, c.n) and tuple(r.accepted.shape) == (O, len(cands))
    assert (r.sims, r.now, r.horizons, r.squeezed) == (sims, now, tuple(horizons), one)
    return _host(r)


PATHS = [(*r, False) for r in PM.RUNS] + [(k, "mixed", True) for k in ("er-small/init", "large/init", "everybody")]


@pytest.mark.parametrize("key,shifts,edge_scan", PATHS)
def test_counts_equal_the_model_on_every_path(key, shifts, edge_scan, dev):
    c = PM.case(key)
    kind = c.base.shape[0] if c.base.shape else key
    if kind == "hubs":
        assert int(np.max(np.diff(c.rp))) > 512                    # rows past GN_SIR_BIGROW
    if kind == "global-lists":
        assert c.n > 11232                                         # the lists do not fit LDS
    if kind == "large":
        assert 2 * c.n > 150 * 1024                                # the scan's state does not fit LDS
    counts, accepted = _run(c, PM.sets_of(key, shifts), getattr(c, shifts), dev, edge_scan=edge_scan)
    want_counts, want_accepted = PM.expected(key, shifts)
    assert np.array_equal(accepted, want_accepted)
    assert np.array_equal(counts, want_counts)


@pytest.mark.parametrize("key,edge_scan", [(k, False) for k in PM.KEYS] + [("er-small/init", True), ("large/init", True)])
def test_lonely_runs_equal_the_model(key, edge_scan, dev):
    """trajectories that end before `now`, between `now` and the last horizon, and never: the final state stays"""
    from gnode.ode_nn import posterior_states_mc
    r = PM.lonely(key)
    c = PM.case(key)
    got = posterior_states_mc(_graph(c), [TM.Observations(r.n, s) for s in r.sets], 0.0, r.gamma, r.sims, r.T, r.now, r.horizons, candidates=r.cands,
                              rng_seed=r.rng_seed, edge_scan=edge_scan, device=dev)
    counts, accepted = _host(got)
    want_counts, want_accepted = PM.lonely_expected(key)
    assert np.array_equal(accepted, want_accepted) and np.array_equal(counts, want_counts)


def test_er_small_equals_one_call_of_the_existing_code_per_candidate(dev):
    """sir_trajectories from the start with the candidate's row replaced, under the phase row moved by the candidate's shift; the
    definition of a matched record and sir_state_at on its event tensors, reduced in torch"""
    import torch
    from gnode.ode_nn import sir_state_at, sir_trajectories
    c = PM.case("er-small/init")
    g = _graph(c)
    sets = PM.sets_of("er-small/init", "mixed")
    now, hz = PM.now_of(c.T), PM.horizons_of(c.T)
    counts, accepted = _run(c, sets, c.mixed, dev)
    want = torch.zeros((len(sets), len(hz), 2, c.n), dtype=torch.int64, device=dev)
    for j, (cand, k) in enumerate(zip(c.cands, c.mixed)):
        p = np.array(c.p)
        if cand >= 0:
            p[cand] = (0.0, 1.0, 0.0)
        beta, gamma = _schedules(c, g, c.phase[k:])
        r = sir_trajectories(g, SC.state(p), beta, gamma, c.sims, c.T, rng_seed=c.rng_seed, events=True, curves=False, device=dev)
        ti, tr = r.t_inf.long(), r.t_rec.long()                     # [sims, n]
        for o, records in enumerate(sets):
            ok = torch.ones(c.sims, dtype=torch.bool, device=ti.device)
            for v, d, kind in records:
                m = now + d
                a, b = ti[:, v], tr[:, v]
                inf, rec = (a >= 0) & (a <= m), (b >= 0) & (b <= m)
                ok &= [~inf, inf & ~rec, rec, a == m, b == m][kind] if m >= 0 else torch.full_like(ok, kind == 0)
            assert int(ok.sum()) == int(accepted[o, j]), (o, j)
            for q, h in enumerate(hz):
                st = sir_state_at(r.t_inf[ok], r.t_rec[ok], now + h)
                want[o, q, 0] += (st == 1).sum(0)
                want[o, q, 1] += (st == 2).sum(0)
    assert np.array_equal(counts, want.cpu().numpy().astype(np.uint64))


def test_the_two_identities(dev):
    """accepted is the top bin of source_scores_timed_mc at age `now`; under the always-matched set everything is accepted and the
    counts summed over the nodes are outbreak_sizes_mc's sums summed over the candidates"""
    from gnode.ode_nn import outbreak_sizes_mc, source_scores_timed_mc
    for key in ("er-small/init", "everybody"):
        c = PM.case(key)
        g = _graph(c)
        beta, gamma = _schedules(c, g)
        sets = PM.sets_of(key, "mixed")
        now, hz = PM.now_of(c.T), PM.horizons_of(c.T)
        counts, accepted = _run(c, sets, c.mixed, dev)
        t = source_scores_timed_mc(g, [TM.Observations(c.n, s) for s in sets], beta, gamma, c.sims, c.T, candidates=c.cands, start=SC.state(c.p),
                                   shifts=c.mixed, rng_seed=c.rng_seed, device=dev)
        assert np.array_equal(accepted, t.hist[:, :, now, t.bins].cpu().numpy().astype(np.uint64))
        assert (accepted[4] == c.sims).all()
        s = outbreak_sizes_mc(g, beta, gamma, c.sims, c.T, candidates=c.cands, start=SC.state(c.p), shifts=c.mixed, rng_seed=c.rng_seed, device=dev)
        sums = s.sums.cpu().numpy().astype(np.uint64)
        for j, h in enumerate(hz):
            assert np.array_equal(counts[4, j].sum(-1), sums[:, now + h, 1:3].sum(0)), (key, h)


def test_two_shards_of_the_sims_range_accumulate_to_the_whole(dev):
    import torch
    c = PM.case("er-small/init")
    sets = PM.sets_of("er-small/init", "mixed")
    want_counts, want_accepted = PM.expected("er-small/init", "mixed")
    cut = 13
    counts = torch.zeros((5, 3, 2, c.n), dtype=torch.int64, device=dev)
    accepted = torch.zeros((5, len(c.cands)), dtype=torch.int64, device=dev)
    a = _run(c, sets, c.mixed, dev, sims=cut, sim_offset=0, counts=counts, accepted=accepted)
    assert not np.array_equal(a[0], want_counts) and (a[1][4] == cut).all()
    b = _run(c, sets, c.mixed, dev, sims=c.sims - cut, sim_offset=cut, counts=counts, accepted=accepted)
    assert np.array_equal(b[0], want_counts) and np.array_equal(b[1], want_accepted)
    rest = _run(c, sets, c.mixed, dev, sims=c.sims - cut, sim_offset=cut)
    assert np.array_equal(rest[0], want_counts - a[0]) and np.array_equal(rest[1], want_accepted - a[1])


def _many_sets(c, key, shifts, count, seed):
    """`count` evidence sets: the case's (a), (d), (e), thinned at random, rotated; the last one is none of the others"""
    base = [PM.sets_of(key, shifts)[i] for i in (0, 3, 4)]
    rng = np.random.default_rng(seed)
    sets = []
    for i in range(count):
        s = [r for r in base[i % 3] if rng.random() >= 0.1 * (i % 5)] or [base[i % 3][0]]
        sets.append(s)
    sets[-1] = [base[0][0], base[0][-1]]
    return sets


def test_seventeen_sets_are_two_groups_and_equal_seventeen_calls(dev):
    c = PM.case("er-small/init")
    sets = _many_sets(c, "er-small/init", "zeros", 17, 17)
    counts, accepted = _run(c, sets, c.zeros, dev)
    for o in range(17):
        one = _run(c, sets[o], c.zeros, dev, one=True)
        assert np.array_equal(counts[o], one[0][0]) and np.array_equal(accepted[o], one[1][0]), o
    first = _run(c, sets[:3], c.zeros, dev)
    assert np.array_equal(counts[:3], first[0]) and np.array_equal(accepted[:3], first[1])
    assert accepted[16].sum() > 0 and not np.array_equal(counts[16], counts[0])


def test_candidate_lists_with_repeats_and_other_orders(dev):
    """accepted[:, c] does not depend on the list; the counts add over the list, a repeated candidate counting twice"""
    c = PM.case("er-small/init")
    sets = PM.sets_of("er-small/init", "mixed")
    want_counts, want_accepted = PM.expected("er-small/init", "mixed")
    singles = [_run(c, sets, [c.mixed[j]], dev, cands=[c.cands[j]]) for j in range(len(c.cands))]
    for j, (cnt, acc) in enumerate(singles):
        assert np.array_equal(acc[:, 0], want_accepted[:, j])
    assert np.array_equal(sum(cnt for cnt, _ in singles), want_counts)
    for pick in ([4, 2], [3, 0, 1, 2, 2, 4, 2], list(range(len(c.cands)))[::-1]):
        cnt, acc = _run(c, sets, [c.mixed[j] for j in pick], dev, cands=[c.cands[j] for j in pick])
        assert np.array_equal(acc, want_accepted[:, pick]) and np.array_equal(cnt, sum(singles[j][0] for j in pick)), pick
    many = list(range(0, c.n, 7)) + [-1]                            # more candidates than workgroups' worth of one: 73 x 3 jobs
    cnt, acc = _run(c, sets, None, dev, cands=many, sims=3)
    one = _run(c, sets, None, dev, cands=[many[11]], sims=3)
    assert np.array_equal(acc[:, 11], one[1][:, 0]) and (acc[4] == 3).all()


def test_defaults_one_object_and_no_trajectories(dev):
    """candidates default to every node, one object drops the set axis in the methods, what gnode.dmp packs is taken as it is;
    sims = 0 touches nothing"""
    import torch
    from gnode.dmp import observations_from_events, timed_observations
    from gnode.ode_nn import posterior_states_mc
    G, n, rp, ci = SC.karate()
    T, sims, now, hz = 8, 50, 4, (0, 2, 3)
    ev = Q.events(n, rp, ci, np.asarray(SC.M.one_hot_init(n, [])), list(range(n)), [0] * n, [np.full(len(ci), 0.2)], [0.3], np.zeros(T, int), sims, T, 3)
    nodes, offsets, kinds = observations_from_events(ev[0][0][1], ev[0][1][1], now, [0, 8, 33], what=("onset", "state"))
    obs = timed_observations(n, nodes, offsets, kinds)
    want_counts, want_accepted = PM.posterior_of(ev, [list(zip(nodes, offsets, kinds))], T, now, hz, n)
    r = posterior_states_mc(G, obs, 0.2, 0.3, sims, T, now, hz, rng_seed=3, device=dev)
    counts, accepted = _host(r)
    assert r.squeezed and np.array_equal(counts, want_counts) and np.array_equal(accepted, want_accepted) and want_accepted[0, 0] >= 1
    tot = int(want_accepted.sum())
    assert int(r.accepted_total()) == tot and tuple(r.source().shape) == (n,) and tuple(r.marginals().shape) == (3, n, 3)
    m = r.marginals().cpu().numpy()
    assert np.allclose(m[..., 1], want_counts[0, :, 0] / tot, rtol=1e-15, atol=0) and np.allclose(m.sum(-1), 1.0, rtol=0, atol=1e-15)
    assert np.allclose(r.source().cpu().numpy(), want_accepted[0] / tot, rtol=1e-15, atol=0)
    for v, d, kind in zip(nodes, offsets, kinds):                   # a sensor's state now is what it reported
        if d == 0 and kind <= 2:
            assert m[0, v, kind] == 1.0
    counts = torch.full((1, 3, 2, n), 7, dtype=torch.int64, device=dev)
    accepted = torch.full((1, n), 7, dtype=torch.int64, device=dev)
    z = posterior_states_mc(G, obs, 0.2, 0.3, 0, T, now, hz, rng_seed=3, counts=counts, accepted=accepted, device=dev)
    assert bool((z.counts == 7).all()) and bool((z.accepted == 7).all()) and z.sims == 0


@pytest.mark.parametrize("edge_scan", [False, True])
def test_the_exact_chain_on_a_graph_with_a_loop(edge_scan, dev):
    """The triangle with a pendant node of tests/test_sir_post_model.py, T = 8, sims = 20 000, (set, now) = (D, 1), (F, 3), (G, 2),
    (D, 0), (F, 4), horizons (0, 1, 3), ONE CALL PER CANDIDATE (the candidates share their coins): every I and R cell within
    5 sqrt(P (1 - P) / sims) + 1 / sims of the forward filter's joint probability, zero where the filter is zero, (D, 0) accepting
    nothing; integer-equal to the model.  On the model the largest share of the bound is 0.515 and 128 cells have P >= 0.01."""
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import posterior_states_mc
    rp, ci = Q.chain_csr()
    g = DeviceGraph(rp, ci)
    worst, cells = 0.0, 0
    for name, now in PM.CHAIN_RUNS:
        obs = TM.Observations(Q.CHAIN_N, TM.CHAIN_SETS[name])
        per = [_host(posterior_states_mc(g, obs, Q.CHAIN_W, Q.CHAIN_GAMMA, PM.CHAIN_SIMS, TM.CHAIN_T, now, PM.CHAIN_HORIZONS, candidates=[cand],
                                         rng_seed=Q.CHAIN_RNG, edge_scan=edge_scan, device=dev)) for cand in range(Q.CHAIN_N)]
        counts, accepted = np.stack([c[0] for c, _ in per]), np.stack([a[0, 0] for _, a in per])
        share, k = PM.check_chain(name, now, counts, accepted)
        worst, cells = max(worst, share), cells + k
        want_counts, want_accepted = PM.chain_counts(name, now)
        assert np.array_equal(counts, want_counts) and np.array_equal(accepted, want_accepted)
        if (name, now) == ("D", 0):
            assert accepted.sum() == 0 and counts.sum() == 0
    print("largest share of the bound", worst, "cells with P >= 0.01", cells)
    assert worst <= 1.0 and cells == 128


def test_the_entry_refuses_and_writes_nothing(dev):
    """through the C entry: O = 0, O = 17, now outside [0, T), H = 0, H = 33, a horizon that is negative, does not ascend or passes
    T - 1, R = 0, a bad set, node, kind and offset, an empty set, what the sweep refuses, null outputs, a short workspace; both
    outputs keep their fill, and a good call after them is served"""
    import ctypes as C
    import torch
    from gnode import _lib
    c = PM.case("er-small/init")
    g = _graph(c)
    lib = _lib.load()
    ARG, WORKSPACE = -1, -3
    n, T, P, L, Cn, sims = c.n, c.T, c.P, c.L, len(c.cands), 4
    now, hz = PM.now_of(T), np.asarray(PM.horizons_of(T), np.int32)
    W, Gm = np.ascontiguousarray(np.stack(c.W)), np.ascontiguousarray(np.stack([np.broadcast_to(x, (n,)) for x in c.G]).astype(np.float64))
    init, phase = np.ascontiguousarray(c.p), np.ascontiguousarray(c.phase)
    cand, shifts = np.asarray(c.cands, np.int32), np.asarray(c.mixed, np.int32)
    sets = PM.sets_of("er-small/init", "mixed")
    rec = np.ascontiguousarray([(o, *r) for o, s in enumerate(sets) for r in s], np.int32)      # [R, 4]: set, node, offset, kind
    R, O, H = len(rec), len(sets), len(hz)
    need = lib.gnode_sir_sweep_posterior_workspace_bytes(g.handle, T, P, L, Cn, O, R, H)
    assert need >= lib.gnode_sir_sweep_workspace_bytes(g.handle, T, P, L, Cn) + 4 * (n + 1) + 4 * R + 2 * O * 4 + 4 * H
    for bad in ((None, T, P, L, Cn, O, R, H), (g.handle, 0, P, L, Cn, O, R, H), (g.handle, T, 0, L, Cn, O, R, H), (g.handle, T, P, T - 1, Cn, O, R, H),
                (g.handle, T, P, L, 0, O, R, H), (g.handle, T, P, L, Cn, 0, R, H), (g.handle, T, P, L, Cn, 17, R, H), (g.handle, T, P, L, Cn, O, 0, H),
                (g.handle, T, P, L, Cn, O, R, 0), (g.handle, T, P, L, Cn, O, R, 33)):
        assert lib.gnode_sir_sweep_posterior_workspace_bytes(*bad) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.full((O, H, 2, n), 7, dtype=torch.int64, device=dev)
    accepted = torch.full((O, Cn), 7, dtype=torch.int64, device=dev)

    def call(init=init, cand=cand, shifts=shifts, Cn=Cn, action=0, phase=phase, P=P, L=L, W=W, Gm=Gm, rec=rec, R=R, O=O, now=now, hz=hz, H=H, sims=sims, T=T,
             nbytes=need, out=counts, acc=accepted):
        hp = lambda a: None if a is None else _lib.host_ptr(a)      # noqa: E731
        cols = [None] * 4 if rec is None else [np.ascontiguousarray(rec[:, j]) for j in range(4)]
        hz32 = None if hz is None else np.ascontiguousarray(hz, np.int32)
        return lib.gnode_sir_mc_philox_sweep_posterior(g.handle, hp(init), hp(cand), hp(shifts), Cn, action, hp(phase), P, L, hp(W), hp(Gm),
                                                       *(hp(x) for x in cols), R, O, now, hp(hz32), H, sims, 0, T, C.c_uint64(c.rng_seed), _lib.ptr(out),
                                                       _lib.ptr(acc), _lib.ptr(ws), nbytes, _lib.stream_ptr(), 0)

    def changed(i, j, value):
        x = rec.copy(); x[i, j] = value
        return x

    said = lambda: lib.gnode_last_error().decode()                  # noqa: E731
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
    assert call(rec=changed(0, 1, -1)) == ARG and "rec_node[0] = -1" in said()
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
    want_counts, want_accepted = PM.expected("er-small/init", "mixed", sims=sims)
    assert np.array_equal(counts.cpu().numpy().astype(np.uint64), want_counts) and np.array_equal(accepted.cpu().numpy().astype(np.uint64), want_accepted)
