"""GPU: Monte-Carlo source scores (gnode_sir_mc_philox_sweep_scores through gnode.ode_nn.source_scores_mc) against
tests/sir_score_model.py, by INTEGER EQUALITY of the histograms, on the cases of tests/sir_sweep_model.py -- lists in LDS, rows
past GN_SIR_BIGROW, lists in the workspace, the scan with its state in LDS and in memory, the everybody-infected branch -- with
three snapshots each (a trajectory's own state, the same partly hidden, a state no trajectory produced), both measures, 64 and
7 bins, no shifts and mixed shifts.  Then against the existing code (one sir_trajectories call per candidate, reduced in torch),
against the sweep's sums, across shards, snapshot groups and candidate lists, against an exact Markov chain on a graph with a
loop, at the largest n that keeps the frontier's lists in LDS next to the tallies, and through the entry's refusals.
tests/test_sir_score_model.py runs the cases' liveness checks and the chain on the CPU."""
import numpy as np
import pytest

import sir_cases as SC
import sir_score_model as Q
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


def _run(c, obs, measure, bins, shifts, dev, cands=None, sims=None, **kw):
    """hist uint64 [O, C, T, bins + 1] of a case through source_scores_mc, as a host array"""
    from gnode.ode_nn import source_scores_mc
    g = _graph(c)
    beta, gamma = _schedules(c, g)
    sims = c.sims if sims is None else sims
    r = source_scores_mc(g, obs, beta, gamma, sims, c.T, candidates=c.cands if cands is None else cands, start=SC.state(c.p), shifts=shifts,
                         measure=measure, bins=bins, rng_seed=c.rng_seed, device=dev, **kw)
    O = 1 if np.ndim(obs) == 1 else len(obs)
    assert r.hist.dtype.is_floating_point is False and tuple(r.hist.shape) == (O, len(c.cands if cands is None else cands), c.T, bins + 1)
    assert (r.sims, r.bins, r.squeezed) == (sims, bins, np.ndim(obs) == 1)
    return r.hist.cpu().numpy().astype(np.uint64)


PATHS = [(*r, False) for r in Q.RUNS] + [(*r, True) for r in Q.RUNS if r[0] in ("er-small/init", "large/init", "everybody")]


@pytest.mark.parametrize("key,measure,bins,shifts,edge_scan", PATHS)
def test_hist_equals_the_model_on_every_path(key, measure, bins, shifts, edge_scan, dev):
    c = Q.case(key)
    kind = c.base.shape[0] if c.base.shape else key
    if kind == "hubs":
        assert int(np.max(np.diff(c.rp))) > 512                    # rows past GN_SIR_BIGROW
    if kind == "global-lists":
        assert c.n > 11232                                         # the lists do not fit LDS
    if kind == "large":
        assert 2 * c.n > 150 * 1024                                # the scan's state does not fit LDS
    got = _run(c, Q.snapshots(key, shifts), measure, bins, getattr(c, shifts), dev, edge_scan=edge_scan)
    assert (got.sum(-1) == c.sims).all()
    assert np.array_equal(got, Q.expected(key, measure, bins, shifts))


@pytest.mark.parametrize("measure,bins", [("jaccard", 64), ("match", 7)])
def test_er_small_equals_one_call_of_the_existing_code_per_candidate(measure, bins, dev):
    """sir_trajectories from the start with the candidate's row replaced, under the phase row moved by the candidate's shift;
    sir_state_at per step, the same integer division and bincount in torch"""
    import torch
    from gnode.ode_nn import sir_state_at, sir_trajectories
    c = Q.case("er-small/init")
    g = _graph(c)
    obs = Q.snapshots("er-small/init", "mixed")
    hist = _run(c, obs, measure, bins, c.mixed, dev)
    ob = torch.from_numpy(np.array(obs)).to(dev)
    for j, (cand, k) in enumerate(zip(c.cands, c.mixed)):
        p = np.array(c.p)
        if cand >= 0:
            p[cand] = (0.0, 1.0, 0.0)
        beta, gamma = _schedules(c, g, c.phase[k:])
        r = sir_trajectories(g, SC.state(p), beta, gamma, c.sims, c.T, rng_seed=c.rng_seed, events=True, curves=False, device=dev)
        for t in range(c.T):
            st = sir_state_at(r.t_inf, r.t_rec, t)                  # int8 [sims, n]
            for o in range(ob.shape[0]):
                seen = ob[o] >= 0
                if measure == "jaccard":
                    A, B = (ob[o] >= 1)[None, :], seen[None, :] & (st != 0)
                    num, den = (A & B).sum(1), (A | B).sum(1)
                else:
                    num, den = (seen[None, :] & (st == ob[o][None, :])).sum(1), seen.sum().expand(st.shape[0])
                kbin = torch.where(den == 0, torch.full_like(num, bins), (num * bins) // den.clamp(min=1))
                want = torch.bincount(kbin, minlength=bins + 1).cpu().numpy().astype(np.uint64)
                assert np.array_equal(hist[o, j, t], want), (o, j, t)


def test_all_ones_under_jaccard_with_n_bins_counts_the_sweeps_sums(dev):
    """one snapshot of all ones, "jaccard", bins = n: the bin of a state is the number of nodes that have left S, so
    sum_k k hist[0, c, t, k] = sums[c, t, 1] + sums[c, t, 2] of outbreak_sizes_mc on the same arguments"""
    from gnode.ode_nn import outbreak_sizes_mc
    c = Q.case("er-small/init")
    g = _graph(c)
    beta, gamma = _schedules(c, g)
    hist = _run(c, np.ones(c.n, np.int8), "jaccard", c.n, c.mixed, dev)
    r = outbreak_sizes_mc(g, beta, gamma, c.sims, c.T, candidates=c.cands, action="seed", start=SC.state(c.p), shifts=c.mixed, rng_seed=c.rng_seed,
                          device=dev)
    sums = r.sums.cpu().numpy().astype(np.uint64)
    left = (hist[0] * np.arange(c.n + 1, dtype=np.uint64)).sum(-1)
    assert np.array_equal(left, sums[:, :, 1] + sums[:, :, 2]) and left.max() > 0


def test_two_shards_of_the_sims_range_accumulate_to_the_whole(dev):
    import torch
    c = Q.case("er-small/init")
    obs, want = Q.snapshots("er-small/init", "mixed"), Q.expected("er-small/init", "jaccard", 64, "mixed")
    cut = 13
    hist = torch.zeros((3, len(c.cands), c.T, 65), dtype=torch.int64, device=dev)
    a = _run(c, obs, "jaccard", 64, c.mixed, dev, sims=cut, sim_offset=0, hist=hist)
    assert not np.array_equal(a, want) and (a.sum(-1) == cut).all()
    b = _run(c, obs, "jaccard", 64, c.mixed, dev, sims=c.sims - cut, sim_offset=cut, hist=hist)
    assert np.array_equal(b, want)
    assert np.array_equal(_run(c, obs, "jaccard", 64, c.mixed, dev, sims=c.sims - cut, sim_offset=cut), want - a)


def test_seventeen_snapshots_are_two_groups_and_equal_seventeen_calls(dev):
    c = Q.case("er-small/init")
    base = Q.snapshots("er-small/init", "zeros")
    rng = np.random.default_rng(17)
    obs = np.stack([np.where(rng.random(c.n) < 0.1 * (i % 5), -1, base[i % 3]) for i in range(17)]).astype(np.int8)
    obs[16] = np.roll(base[0], 1)                                   # the snapshot alone in the second group is none of the first's
    assert all((obs[i] >= 0).any() for i in range(17))
    for measure, bins in (("match", 64), ("jaccard", 7)):
        got = _run(c, obs, measure, bins, c.zeros, dev)
        for o in range(17):
            assert np.array_equal(got[o], _run(c, obs[o], measure, bins, c.zeros, dev)[0]), (measure, o)
        assert np.array_equal(got[:3], _run(c, obs[:3], measure, bins, c.zeros, dev))
        assert not np.array_equal(got[16], got[0])


def test_a_candidates_rows_do_not_depend_on_the_list(dev):
    """alone, at another position, next to other neighbours, in a list of other length: the same rows"""
    c = Q.case("er-small/init")
    obs, want = Q.snapshots("er-small/init", "mixed"), Q.expected("er-small/init", "match", 64, "mixed")
    for pick in ([2], [4, 2], [3, 0, 5 % len(c.cands), 1, 2, 2, 4], list(range(len(c.cands)))[::-1]):
        got = _run(c, obs, "match", 64, [c.mixed[j] for j in pick], dev, cands=[c.cands[j] for j in pick])
        assert np.array_equal(got, want[:, pick]), pick
    many = list(range(0, c.n, 7)) + [-1]                            # more candidates than workgroups' worth of one: 73 x 3 jobs
    got = _run(c, obs, "match", 64, None, dev, cands=many, sims=3)
    one = _run(c, obs, "match", 64, None, dev, cands=[many[11]], sims=3)
    assert np.array_equal(got[:, 11], one[:, 0]) and (got.sum(-1) == 3).all()


def test_defaults_and_no_trajectories(dev):
    """candidates default to every node, one snapshot gives [C, T] tables that rank_sources reads; sims = 0 touches nothing"""
    import torch
    from gnode.dmp import rank_sources
    from gnode.ode_nn import source_scores_mc
    G, n, rp, ci = SC.karate()
    want = Q.scores(n, rp, ci, np.asarray(SC.M.one_hot_init(n, [])), list(range(n)), [0] * n, [np.full(len(ci), 0.2)], [0.3], np.zeros(8, int),
                    np.ones(n, np.int8), "jaccard", 64, 50, 8, 3)
    obs = torch.ones(n, dtype=torch.int8, device=dev)               # a tensor on the device is copied to the host
    r = source_scores_mc(G, obs, 0.2, 0.3, 50, 8, rng_seed=3, device=dev)
    assert tuple(r.hist.shape) == (1, n, 8, 65) and r.squeezed and np.array_equal(r.hist.cpu().numpy().astype(np.uint64), want)
    assert tuple(r.scores().shape) == (n, 8) == tuple(r.exact().shape) and r.scores().dtype == torch.float64
    assert np.allclose(r.scores(0.3).cpu().numpy(), Q.kernel_scores(want[0], 50, 0.3), rtol=1e-12, atol=0)
    assert len(rank_sources(r.scores(), list(range(n)))) == n
    hist = torch.full((1, n, 8, 65), 7, dtype=torch.int64, device=dev)
    z = source_scores_mc(G, obs, 0.2, 0.3, 0, 8, rng_seed=3, hist=hist, device=dev)
    assert bool((z.hist == 7).all()) and z.sims == 0


def test_the_exact_chain_on_a_graph_with_a_loop(dev):
    """The triangle with a pendant node of tests/test_sir_score_model.py, sims = 20 000: the top bin of "match" against the
    81-state chain's P(c, t), within 5 sqrt(P (1 - P) / sims) + 1 / sims in every cell, zero where the chain is zero, and
    the same argmax (c = 0, t = 2)."""
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import source_scores_mc
    from test_sir_score_model import chain_table, check_chain
    rp, ci = Q.chain_csr()
    sims = 20_000
    r = source_scores_mc(DeviceGraph(rp, ci), Q.CHAIN_OBS, Q.CHAIN_W, Q.CHAIN_GAMMA, sims, Q.CHAIN_T, measure="match", bins=4, rng_seed=Q.CHAIN_RNG,
                         device=dev)
    hist = r.hist.cpu().numpy().astype(np.uint64)[0]
    check_chain(hist, sims, chain_table())
    assert np.array_equal(hist, Q.chain_hist(sims))
    assert np.allclose(r.exact().cpu().numpy(), hist[:, :, 4] / sims, rtol=1e-14, atol=0)     # (float64; the device may scale by 1 / sims)


def test_the_largest_graph_with_its_lists_in_lds_next_to_sixteen_snapshots(dev):
    """n = 11 200: bitmaps (4 224 bytes) + uint16 lists (44 800) + the tallies of 16 snapshots (128) are the 48 KiB of the
    lists-in-LDS form exactly (tests/test_sir_score_plan.py: 11 201 goes to the workspace); 2 candidates, 8 sims, O = 16"""
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import source_scores_mc
    n, m, T, sims, seeds, cands = 11200, 30000, 6, 8, list(range(7, 11200, 500)), [5, -1]
    assert 3 * ((((n + 31) // 32) + 3) // 4 * 4) * 4 + 2 * 2 * n + 2 * Q.MAXO * 4 == 48 * 1024
    rp, ci = SC.csr("score-lds-boundary", n, m)
    assert int(np.max(np.diff(rp))) <= 512
    p = np.asarray(SC.M.one_hot_init(n, seeds))
    W, G, phase = [np.full(len(ci), 0.3)], [0.2], np.zeros(T, np.int32)
    ev = Q.events(n, rp, ci, p, cands, [0, 0], W, G, phase, sims, T, 77)
    rng = np.random.default_rng(1)
    obs = np.stack([np.where(rng.random(n) < 0.05 * (i // 6), -1, Q.states_at(ev[i % 2][0][i % sims:i % sims + 1], ev[i % 2][1][i % sims:i % sims + 1], i % T)[0])
                    for i in range(Q.MAXO)]).astype(np.int8)
    for measure, bins in (("jaccard", 64), ("match", 4096)):
        want = Q.hist_of(ev, obs, measure, bins, T)
        r = source_scores_mc(DeviceGraph(rp, ci), obs, 0.3, 0.2, sims, T, candidates=cands, start=seeds, measure=measure, bins=bins, rng_seed=77, device=dev)
        got = r.hist.cpu().numpy().astype(np.uint64)
        assert np.array_equal(got, want) and want[:, :, :, bins].sum() >= Q.MAXO and want[:, :, :, 1:bins].sum() > 0


def test_the_entry_refuses_and_writes_nothing(dev):
    """through the C entry: a bad code, O = 0, O = 17, bins = 0, a bad measure, a blind snapshot, too many cells, what the sweep
    refuses, a short workspace; hist keeps its fill, and a good call after them is served"""
    import ctypes as C
    import torch
    from gnode import _lib
    c = Q.case("er-small/init")
    g = _graph(c)
    lib = _lib.load()
    ARG, WORKSPACE = -1, -3
    n, T, P, L, Cn, sims, bins = c.n, c.T, c.P, c.L, len(c.cands), 4, 64
    W, Gm = np.ascontiguousarray(np.stack(c.W)), np.ascontiguousarray(np.stack([np.broadcast_to(x, (n,)) for x in c.G]).astype(np.float64))
    init, phase = np.ascontiguousarray(c.p), np.ascontiguousarray(c.phase)
    cand, shifts = np.asarray(c.cands, np.int32), np.asarray(c.mixed, np.int32)
    obs = np.ascontiguousarray(Q.snapshots("er-small/init", "mixed"))
    need = lib.gnode_sir_sweep_scores_workspace_bytes(g.handle, T, P, L, Cn, 3)
    assert need >= lib.gnode_sir_sweep_workspace_bytes(g.handle, T, P, L, Cn) + 3 * n + 2 * 3 * 4
    for bad in ((None, T, P, L, Cn, 3), (g.handle, 0, P, L, Cn, 3), (g.handle, T, 0, L, Cn, 3), (g.handle, T, P, T - 1, Cn, 3), (g.handle, T, P, L, 0, 3),
                (g.handle, T, P, L, Cn, 0), (g.handle, T, P, L, Cn, 17)):
        assert lib.gnode_sir_sweep_scores_workspace_bytes(*bad) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    hist = torch.full((3, Cn, T, bins + 1), 7, dtype=torch.int64, device=dev)

    def call(init=init, cand=cand, shifts=shifts, Cn=Cn, action=0, phase=phase, P=P, L=L, W=W, Gm=Gm, obs=obs, O=3, measure=0, bins=bins, sims=sims, T=T,
             nbytes=need, out=hist):
        hp = lambda a: None if a is None else _lib.host_ptr(a)      # noqa: E731
        return lib.gnode_sir_mc_philox_sweep_scores(g.handle, hp(init), hp(cand), hp(shifts), Cn, action, hp(phase), P, L, hp(W), hp(Gm), hp(obs), O,
                                                    measure, bins, sims, 0, T, C.c_uint64(c.rng_seed), _lib.ptr(out), _lib.ptr(ws), nbytes,
                                                    _lib.stream_ptr(), 0)

    said = lambda: lib.gnode_last_error().decode()                  # noqa: E731
    x = obs.copy(); x[1, 9] = 3
    assert call(obs=x) == ARG and "obs[1][9] = 3" in said()
    x = obs.copy(); x[2, 0] = -2
    assert call(obs=x) == ARG and "obs[2][0] = -2" in said()
    assert call(O=0) == ARG and "O = 0" in said()
    assert call(O=17) == ARG and "O = 17" in said()
    assert call(bins=0) == ARG and "bins = 0" in said()
    assert call(bins=4097) == ARG and call(measure=2) == ARG and call(measure=-1) == ARG
    x = obs.copy(); x[0] = -1
    assert call(obs=x) == ARG and "snapshot 0 observes no node" in said()
    assert call(bins=4096, T=1, Cn=200_000) == ARG and "2^31" in said()       # (refused before the candidates are read)
    assert call(obs=None) == ARG and call(out=None) == ARG and call(init=None) == ARG
    x = shifts.copy(); x[3] = L - T + 1
    assert call(shifts=x) == ARG and f"shifts[3] = {L - T + 1}" in said()
    assert call(Cn=0) == ARG and call(action=2) == ARG and call(L=T - 1) == ARG and call(P=0) == ARG and call(sims=-1) == ARG and call(T=0) == ARG
    assert call(nbytes=need - 1) == WORKSPACE
    assert call(sims=0) == 0, said()                                # valid, and touches nothing
    torch.cuda.synchronize()
    assert bool((hist == 7).all())
    hist.zero_()
    assert call() == 0, said()
    assert np.array_equal(hist.cpu().numpy().astype(np.uint64), Q.expected("er-small/init", "jaccard", 64, "mixed", sims=sims))
