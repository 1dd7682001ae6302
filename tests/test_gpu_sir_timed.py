"""GPU: Monte-Carlo source scores from timed evidence (gnode_sir_mc_philox_sweep_timed through
gnode.ode_nn.source_scores_timed_mc) against tests/sir_timed_model.py, by INTEGER EQUALITY of the histograms, on the cases of
tests/sir_sweep_model.py -- lists in LDS, rows past GN_SIR_BIGROW, lists in the workspace, the scan with its state in LDS and in
memory, the everybody-infected branch -- with three evidence sets each (what sensors report of a trajectory, the same with a
record further back than T, a repeated node and a candidate among the sensors, a set no trajectory satisfies), the default
bins and 5, mixed shifts and none.  Then against the existing code (one sir_trajectories call per candidate, reduced in torch
by the definition), against source_scores_mc where the two must coincide, across shards, set groups and candidate lists,
against an exact forward filter on a graph with a loop, and through the entry's refusals.  tests/test_sir_timed_model.py runs
the cases' liveness checks and the chain on the CPU."""
import numpy as np
import pytest

import sir_cases as SC
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


def _run(c, sets, bins, shifts, dev, cands=None, sims=None, one=False, **kw):
    """hist uint64 [O, C, T, bins + 1] of a case through source_scores_timed_mc, as a host array; one: `sets` is one set of
    records, given as one object"""
    from gnode.ode_nn import source_scores_timed_mc
    g = _graph(c)
    beta, gamma = _schedules(c, g)
    sims = c.sims if sims is None else sims
    obs = TM.Observations(c.n, sets) if one else [TM.Observations(c.n, s) for s in sets]
    r = source_scores_timed_mc(g, obs, beta, gamma, sims, c.T, candidates=c.cands if cands is None else cands, start=SC.state(c.p), shifts=shifts,
                               bins=bins, rng_seed=c.rng_seed, device=dev, **kw)
    B = max(len(s) for s in ([sets] if one else sets)) if bins is None else bins
    assert r.hist.dtype.is_floating_point is False and tuple(r.hist.shape) == (1 if one else len(sets), len(c.cands if cands is None else cands), c.T, B + 1)
    assert (r.sims, r.bins, r.squeezed) == (sims, B, one)
    return r.hist.cpu().numpy().astype(np.uint64)


BINS = {"mixed": None, "zeros": 5}
PATHS = [(*r, False) for r in TM.RUNS] + [(*r, True) for r in TM.RUNS if r[0] in ("er-small/init", "large/init", "everybody")]


@pytest.mark.parametrize("key,shifts,edge_scan", PATHS)
def test_hist_equals_the_model_on_every_path(key, shifts, edge_scan, dev):
    c = TM.case(key)
    kind = c.base.shape[0] if c.base.shape else key
    if kind == "hubs":
        assert int(np.max(np.diff(c.rp))) > 512                    # rows past GN_SIR_BIGROW
    if kind == "global-lists":
        assert c.n > 11232                                         # the lists do not fit LDS
    if kind == "large":
        assert 2 * c.n > 150 * 1024                                # the scan's state does not fit LDS
    got = _run(c, TM.evidence(key, shifts), BINS[shifts], getattr(c, shifts), dev, edge_scan=edge_scan)
    assert (got.sum(-1) == c.sims).all()
    assert np.array_equal(got, TM.expected(key, shifts, BINS[shifts]))


def test_er_small_equals_one_call_of_the_existing_code_per_candidate(dev):
    """sir_trajectories from the start with the candidate's row replaced, under the phase row moved by the candidate's shift; the
    definition of a matched record on its event tensors, the same integer division and bincount in torch"""
    import torch
    from gnode.ode_nn import sir_trajectories
    c = TM.case("er-small/init")
    g = _graph(c)
    sets = TM.evidence("er-small/init", "mixed")
    for bins in (None, 5):
        hist = _run(c, sets, bins, c.mixed, dev)
        B = hist.shape[-1] - 1
        for j, (cand, k) in enumerate(zip(c.cands, c.mixed)):
            p = np.array(c.p)
            if cand >= 0:
                p[cand] = (0.0, 1.0, 0.0)
            beta, gamma = _schedules(c, g, c.phase[k:])
            r = sir_trajectories(g, SC.state(p), beta, gamma, c.sims, c.T, rng_seed=c.rng_seed, events=True, curves=False, device=dev)
            ti, tr = r.t_inf.long(), r.t_rec.long()                 # [sims, n]
            for o, records in enumerate(sets):
                agree = torch.zeros((c.sims, c.T), dtype=torch.int64, device=ti.device)
                for v, d, kind in records:
                    m = (torch.arange(c.T, device=ti.device) + d)[None, :]
                    a, b = ti[:, v][:, None], tr[:, v][:, None]
                    inf, rec = (a >= 0) & (a <= m), (b >= 0) & (b <= m)
                    at = [~inf, inf & ~rec, rec, a == m, b == m][kind]
                    agree += torch.where(m < 0, torch.full_like(at, kind == 0), at).long()
                kbin = (agree * B) // len(records)
                for t in range(c.T):
                    want = torch.bincount(kbin[:, t], minlength=B + 1).cpu().numpy().astype(np.uint64)
                    assert np.array_equal(hist[o, j, t], want), (o, j, t)


def test_states_now_are_source_scores_mc_under_match(dev):
    """a set with all its records at offset 0 and kinds 0 to 2 IS a snapshot: integer for integer the histogram of
    source_scores_mc(measure="match") with the same bins"""
    from gnode.ode_nn import source_scores_mc
    c = TM.case("er-small/init")
    g = _graph(c)
    beta, gamma = _schedules(c, g)
    snaps = Q.snapshots("er-small/init", "mixed")[1:]               # partly hidden; a state no trajectory produced
    sets = [[(int(v), 0, int(s[v])) for v in np.flatnonzero(s >= 0)] for s in snaps]
    for bins in (64, 7):
        got = _run(c, sets, bins, c.mixed, dev)
        r = source_scores_mc(g, snaps, beta, gamma, c.sims, c.T, candidates=c.cands, start=SC.state(c.p), shifts=c.mixed, measure="match", bins=bins,
                             rng_seed=c.rng_seed, device=dev)
        assert np.array_equal(got, r.hist.cpu().numpy().astype(np.uint64)) and got[0, :, :, bins].sum() >= 1


def test_two_shards_of_the_sims_range_accumulate_to_the_whole(dev):
    import torch
    c = TM.case("er-small/init")
    sets, want = TM.evidence("er-small/init", "mixed"), TM.expected("er-small/init", "mixed")
    cut, B = 13, want.shape[-1] - 1
    hist = torch.zeros((3, len(c.cands), c.T, B + 1), dtype=torch.int64, device=dev)
    a = _run(c, sets, None, c.mixed, dev, sims=cut, sim_offset=0, hist=hist)
    assert not np.array_equal(a, want) and (a.sum(-1) == cut).all()
    b = _run(c, sets, None, c.mixed, dev, sims=c.sims - cut, sim_offset=cut, hist=hist)
    assert np.array_equal(b, want)
    assert np.array_equal(_run(c, sets, None, c.mixed, dev, sims=c.sims - cut, sim_offset=cut), want - a)


def _many_sets(c, key, shifts, count, seed):
    """`count` evidence sets: the case's three, thinned at random, rotated; the last one is none of the others"""
    base = TM.evidence(key, shifts)
    rng = np.random.default_rng(seed)
    sets = []
    for i in range(count):
        s = [r for r in base[i % 3] if rng.random() >= 0.1 * (i % 5)] or [base[i % 3][0]]
        sets.append(s)
    sets[-1] = [((v + 1) % c.n, d, kind) for v, d, kind in base[0]]
    return sets


def test_seventeen_sets_are_two_groups_and_equal_seventeen_calls(dev):
    c = TM.case("er-small/init")
    sets = _many_sets(c, "er-small/init", "zeros", 17, 17)
    for bins in (8, 3):                                             # (one bin count for all sets: a set alone would default to its own)
        got = _run(c, sets, bins, c.zeros, dev)
        for o in range(17):
            assert np.array_equal(got[o], _run(c, sets[o], bins, c.zeros, dev, one=True)[0]), (bins, o)
        assert np.array_equal(got[:3], _run(c, sets[:3], bins, c.zeros, dev))
        assert not np.array_equal(got[16], got[0])


def test_a_long_run_takes_fewer_sets_per_launch(dev):
    """maxTime = 130: 2048 // 130 = 15 sets share a launch, the sixteenth runs alone; 8 sims; equal to the single calls and to
    the model"""
    from gnode.ode_nn import source_scores_timed_mc
    G, n, rp, ci = SC.karate()
    T, sims, cands, w, gamma, rng_seed = 130, 8, [0, 33, -1, 5], 0.05, 0.04, 21
    assert TM.CELLS // T < 16
    ev = Q.events(n, rp, ci, np.asarray(SC.M.one_hot_init(n, [])), cands, [0] * 4, [np.full(len(ci), w)], [gamma], np.zeros(T, int), sims, T, rng_seed)
    t_inf, t_rec = ev[0][0][0], ev[0][1][0]
    assert t_rec.max() == T - 1 and ev[0][0].max() >= 80            # the runs are still going late: an event in the last cell
    sets = [TM.reports(t_inf, t_rec, 20 + 7 * o, list(range(o % 4, n, 4))) + [(o, -(T - 1), 0), (o, -T, 0)] for o in range(16)]
    obs = [TM.Observations(n, s) for s in sets]
    r = source_scores_timed_mc(G, obs, w, gamma, sims, T, candidates=cands, bins=6, rng_seed=rng_seed, device=dev)
    got = r.hist.cpu().numpy().astype(np.uint64)
    assert np.array_equal(got, TM.hist_of(ev, sets, 6, T)) and got[:, 0, :, 6].sum() >= 16
    for o in (0, 14, 15):
        one = source_scores_timed_mc(G, obs[o], w, gamma, sims, T, candidates=cands, bins=6, rng_seed=rng_seed, device=dev)
        assert one.squeezed and np.array_equal(one.hist.cpu().numpy().astype(np.uint64)[0], got[o])


def test_a_candidates_rows_do_not_depend_on_the_list(dev):
    """alone, at another position, next to other neighbours, in a list of other length: the same rows"""
    c = TM.case("er-small/init")
    sets, want = TM.evidence("er-small/init", "mixed"), TM.expected("er-small/init", "mixed")
    for pick in ([2], [4, 2], [3, 0, 5 % len(c.cands), 1, 2, 2, 4], list(range(len(c.cands)))[::-1]):
        got = _run(c, sets, None, [c.mixed[j] for j in pick], dev, cands=[c.cands[j] for j in pick])
        assert np.array_equal(got, want[:, pick]), pick
    many = list(range(0, c.n, 7)) + [-1]                            # more candidates than workgroups' worth of one: 73 x 3 jobs
    got = _run(c, sets, None, None, dev, cands=many, sims=3)
    one = _run(c, sets, None, None, dev, cands=[many[11]], sims=3)
    assert np.array_equal(got[:, 11], one[:, 0]) and (got.sum(-1) == 3).all()


def test_defaults_and_no_trajectories(dev):
    """candidates default to every node, one object gives [C, T] tables that rank_sources reads, what gnode.dmp packs is taken
    as it is; sims = 0 touches nothing"""
    import torch
    from gnode.dmp import observations_from_events, rank_sources, timed_observations
    from gnode.ode_nn import source_scores_timed_mc
    G, n, rp, ci = SC.karate()
    T, sims = 8, 50
    ev = Q.events(n, rp, ci, np.asarray(SC.M.one_hot_init(n, [])), list(range(n)), [0] * n, [np.full(len(ci), 0.2)], [0.3], np.zeros(T, int), sims, T, 3)
    nodes, offsets, kinds = observations_from_events(ev[0][0][1], ev[0][1][1], 4, [0, 1, 2, 8, 13, 33], what=("onset", "removal", "state"))
    obs = timed_observations(n, nodes, offsets, kinds)
    records = list(zip(nodes, offsets, kinds))
    want = TM.hist_of(ev, [records], len(records), T)
    r = source_scores_timed_mc(G, obs, 0.2, 0.3, sims, T, rng_seed=3, device=dev)
    assert tuple(r.hist.shape) == (1, n, T, len(records) + 1) and r.squeezed and np.array_equal(r.hist.cpu().numpy().astype(np.uint64), want)
    assert want[0, 0, 4, len(records)] >= 1                         # the trajectory that reported is found at its source and age
    assert tuple(r.scores().shape) == (n, T) == tuple(r.exact().shape) and r.scores().dtype == torch.float64
    assert np.allclose(r.scores(0.3).cpu().numpy(), Q.kernel_scores(want[0], sims, 0.3), rtol=1e-12, atol=0)
    assert len(rank_sources(r.scores(), list(range(n)))) == n
    hist = torch.full((1, n, T, len(records) + 1), 7, dtype=torch.int64, device=dev)
    z = source_scores_timed_mc(G, obs, 0.2, 0.3, 0, T, rng_seed=3, hist=hist, device=dev)
    assert bool((z.hist == 7).all()) and z.sims == 0


def test_the_exact_chain_on_a_graph_with_a_loop(dev):
    """The triangle with a pendant node of tests/test_sir_timed_model.py, T = 8, sims = 20 000, the sets D, F and G: the top bin
    against the forward filter's P(all records | c, t), within 5 sqrt(P (1 - P) / sims) + 1 / sims in every cell, zero where the
    filter is zero, the same argmax, at least 30 cells with P >= 0.01 in all"""
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import source_scores_timed_mc
    rp, ci = Q.chain_csr()
    sims = 20_000
    obs = [TM.Observations(Q.CHAIN_N, TM.CHAIN_SETS[k]) for k in "DFG"]
    r = source_scores_timed_mc(DeviceGraph(rp, ci), obs, Q.CHAIN_W, Q.CHAIN_GAMMA, sims, TM.CHAIN_T, rng_seed=Q.CHAIN_RNG, device=dev)
    assert r.bins == 3 and not r.squeezed
    hist = r.hist.cpu().numpy().astype(np.uint64)
    TM.check_chain(hist, sims)
    assert np.array_equal(hist, TM.chain_hist(sims))
    assert np.allclose(r.exact().cpu().numpy(), hist[:, :, :, 3] / sims, rtol=1e-14, atol=0)  # (float64; the device may scale by 1 / sims)


def test_the_entry_refuses_and_writes_nothing(dev):
    """through the C entry: O = 0, O = 17, too many cells, bins = 0, R = 0, a bad set, node, kind and offset, an empty set, too
    many histogram cells, what the sweep refuses, a short workspace; hist keeps its fill, and a good call after them is served"""
    import ctypes as C
    import torch
    from gnode import _lib
    c = TM.case("er-small/init")
    g = _graph(c)
    lib = _lib.load()
    ARG, WORKSPACE = -1, -3
    n, T, P, L, Cn, sims, bins = c.n, c.T, c.P, c.L, len(c.cands), 4, 5
    W, Gm = np.ascontiguousarray(np.stack(c.W)), np.ascontiguousarray(np.stack([np.broadcast_to(x, (n,)) for x in c.G]).astype(np.float64))
    init, phase = np.ascontiguousarray(c.p), np.ascontiguousarray(c.phase)
    cand, shifts = np.asarray(c.cands, np.int32), np.asarray(c.mixed, np.int32)
    sets = TM.evidence("er-small/init", "mixed")
    rec = np.ascontiguousarray([(o, *r) for o, s in enumerate(sets) for r in s], np.int32)      # [R, 4]: set, node, offset, kind
    R = len(rec)
    need = lib.gnode_sir_sweep_timed_workspace_bytes(g.handle, T, P, L, Cn, 3, R)
    assert need >= lib.gnode_sir_sweep_workspace_bytes(g.handle, T, P, L, Cn) + 4 * (n + 1) + 4 * R + 2 * 3 * 4
    for bad in ((None, T, P, L, Cn, 3, R), (g.handle, 0, P, L, Cn, 3, R), (g.handle, T, 0, L, Cn, 3, R), (g.handle, T, P, T - 1, Cn, 3, R),
                (g.handle, T, P, L, 0, 3, R), (g.handle, T, P, L, Cn, 0, R), (g.handle, T, P, L, Cn, 17, R), (g.handle, T, P, L, Cn, 3, 0)):
        assert lib.gnode_sir_sweep_timed_workspace_bytes(*bad) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    hist = torch.full((3, Cn, T, bins + 1), 7, dtype=torch.int64, device=dev)

    def call(init=init, cand=cand, shifts=shifts, Cn=Cn, action=0, phase=phase, P=P, L=L, W=W, Gm=Gm, rec=rec, R=R, O=3, bins=bins, sims=sims, T=T,
             nbytes=need, out=hist):
        hp = lambda a: None if a is None else _lib.host_ptr(a)      # noqa: E731
        cols = [None] * 4 if rec is None else [np.ascontiguousarray(rec[:, j]) for j in range(4)]
        return lib.gnode_sir_mc_philox_sweep_timed(g.handle, hp(init), hp(cand), hp(shifts), Cn, action, hp(phase), P, L, hp(W), hp(Gm), *(hp(x) for x in cols),
                                                   R, O, bins, sims, 0, T, C.c_uint64(c.rng_seed), _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_ptr(), 0)

    def changed(i, j, value):
        x = rec.copy(); x[i, j] = value
        return x

    said = lambda: lib.gnode_last_error().decode()                  # noqa: E731
    assert call(O=0) == ARG and "O = 0" in said()
    assert call(O=17) == ARG and "O = 17" in said()
    assert call(O=3, T=700, L=700) == ARG and "2048" in said()      # (refused before the phase row is read)
    assert call(bins=0) == ARG and "bins = 0" in said()
    assert call(bins=4097) == ARG and call(R=0) == ARG and "R = 0" in said()
    assert call(rec=changed(7, 0, 3)) == ARG and "rec_set[7] = 3" in said()
    assert call(rec=changed(9, 1, n)) == ARG and f"rec_node[9] = {n}" in said()
    assert call(rec=changed(0, 1, -1)) == ARG and "rec_node[0] = -1" in said()
    assert call(rec=changed(2, 3, 5)) == ARG and "rec_kind[2] = 5" in said()
    assert call(rec=changed(R - 1, 2, 1)) == ARG and f"rec_offset[{R - 1}] = 1" in said()
    assert call(rec=rec[rec[:, 0] != 1], R=int((rec[:, 0] != 1).sum())) == ARG and "evidence set 1 holds no record" in said()
    assert call(bins=4096, T=1, Cn=200_000) == ARG and "2^31" in said()       # (refused before the candidates are read)
    assert call(rec=None) == ARG and call(out=None) == ARG and call(init=None) == ARG
    x = shifts.copy(); x[3] = L - T + 1
    assert call(shifts=x) == ARG and f"shifts[3] = {L - T + 1}" in said()
    assert call(Cn=0) == ARG and call(action=2) == ARG and call(L=T - 1) == ARG and call(P=0) == ARG and call(sims=-1) == ARG and call(T=0) == ARG
    assert call(nbytes=need - 1) == WORKSPACE
    assert call(sims=0) == 0, said()                                # valid, and touches nothing
    torch.cuda.synchronize()
    assert bool((hist == 7).all())
    hist.zero_()
    assert call() == 0, said()
    assert np.array_equal(hist.cpu().numpy().astype(np.uint64), TM.expected("er-small/init", "mixed", bins, sims=sims))
