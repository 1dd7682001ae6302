"""The CPU model of the Monte-Carlo nowcast and forecast from timed evidence (`gnode_sir_mc_philox_sweep_posterior`,
`posterior_states_mc`) and its cases, stated once (a helper, not a test).  numpy only.

The trajectories and the records are those of tests/sir_timed_model.py.  With `now` the age at which the records are anchored,
trajectory (c, s) is ACCEPTED for an evidence set when every record of the set is matched at age `now`:
`agree_of(...)[:, now] == len(records)`.  accepted[o, c] counts the accepted trajectories of candidate c; counts[o, j, 0, v]
counts, over the accepted trajectories of ALL candidates, those in which node v is I at step now + horizons[j], and
counts[o, j, 1, v] those in which it is R (`states_at`: a trajectory that ended early keeps its final state).
`posterior_of` is that definition; `agree_now_by_counter` restates the kernels' one counter per set, the difference array of
tests/sir_timed_model.py summed up to cell `now`.

The cases are those of tests/sir_timed_model.py (`RUNS`) at now = T // 2 with the horizons {0, 1, T - 1 - now} and five
evidence sets (`sets_of`): that module's (a), (b), (c); (d) = the first record of (a) with a record further back than T, which
many trajectories satisfy; (e) = that always-matched record alone, which every trajectory satisfies.  `lonely` adds, on every
case's graph, a run in which nothing spreads (every contact probability 0, gamma 0.3, nobody infected but the candidate), so
that trajectories end before `now`, between `now` and the last horizon, and never."""
import functools

import numpy as np

import sir_cases as SC
import sir_score_model as Q
import sir_timed_model as TM

MAXO, MAXH = TM.MAXO, 32                                            # GN_SIR_SCORE_MAXO, GN_SIR_POST_MAXH of the library as built by default


def accepted_rows(t_inf, t_rec, records, T, now):
    """bool [sims]: every record of the set is matched at age `now`, by the definition"""
    return TM.agree_of(t_inf, t_rec, records, T)[:, now] == len(records)


def posterior_of(events, sets, T, now, horizons, n):
    """(counts uint64 [O, H, 2, n], accepted uint64 [O, C]) from the per-candidate events [(t_inf, t_rec)], by the definition"""
    counts = np.zeros((len(sets), len(horizons), 2, n), dtype=np.uint64)
    accepted = np.zeros((len(sets), len(events)), dtype=np.uint64)
    for o, records in enumerate(sets):
        for c, (t_inf, t_rec) in enumerate(events):
            ok = accepted_rows(t_inf, t_rec, records, T, now)
            accepted[o, c] = ok.sum()
            for j, h in enumerate(horizons):
                st = Q.states_at(t_inf[ok], t_rec[ok], now + int(h))
                counts[o, j, 0] += (st == 1).sum(0).astype(np.uint64)
                counts[o, j, 1] += (st == 2).sum(0).astype(np.uint64)
    return counts, accepted


def agree_now_by_counter(t_inf, t_rec, records, T, now):
    """int64 [sims], as the kernels count it: from the number of kind-0 records on, a node's infection at step `it` moves the
    counter of a record (kind, back = min(-d, T)) on that node, pos = it + back, by -1 (kind 0) or +1 (kind 1) iff pos <= now and
    by +1 (kind 3) iff pos == now; its recovery by -1 (kind 1) or +1 (kind 2) iff pos <= now and by +1 (kind 4) iff pos == now"""
    t_inf, t_rec = np.asarray(t_inf).astype(np.int64), np.asarray(t_rec).astype(np.int64)
    agr = np.full(t_inf.shape[0], sum(int(r[2]) == 0 for r in records), dtype=np.int64)
    for v, d, kind in records:
        back = min(-int(d), T)
        for which, (when, steps) in enumerate(((t_inf[:, v], {0: -1, 1: +1}), (t_rec[:, v], {1: -1, 2: +1}))):
            pos = when + back
            if kind in steps:
                agr += steps[kind] * ((when >= 0) & (pos <= now))
            if kind == 3 + which:
                agr += (when >= 0) & (pos == now)
    return agr


def end_step(t_inf, t_rec, T):
    """int64 [sims]: the step after which nobody is infected (0: nobody ever was), or T where somebody still is at step T - 1"""
    t_inf, t_rec = np.asarray(t_inf).astype(np.int64), np.asarray(t_rec).astype(np.int64)
    still = ((t_inf >= 0) & (t_rec < 0)).any(1)
    return np.where(still, T, np.maximum(t_rec.max(1), 0))


# ----------------------------------------------------------------------------------------------------------------- cases
KEYS, RUNS = TM.KEYS, TM.RUNS
case, case_events = TM.case, TM.case_events


def now_of(T):
    return T // 2


def horizons_of(T):
    return sorted({0, 1, T - 1 - now_of(T)})


@functools.lru_cache(maxsize=None)
def sets_of(key, shifts):
    """((a), (b), (c), (d), (e)) of the module's text"""
    c = case(key)
    a, b, cset = TM.evidence(key, shifts)
    always = (a[0][0], -(c.T + 3), 0)
    return a, b, cset, (a[0], always), (always,)


@functools.lru_cache(maxsize=None)
def expected(key, shifts, sims=None, sim_offset=0):
    """(counts, accepted) of the model for a case against its five sets, read-only"""
    c = case(key)
    out = posterior_of(case_events(key, shifts, sims, sim_offset), sets_of(key, shifts), c.T, now_of(c.T), horizons_of(c.T), c.n)
    return tuple(SC._frozen(x) for x in out)


def live(key, shifts):
    """On the model's own output: (a) and (b) accept 1 to 12 jobs, (c) none, (d) 5 to 140, (e) all; no count exceeds the accepted
    total and some node is counted in each plane of (e); the counter form gives the same acceptances; only `everybody` has
    accepted trajectories that end before the last horizon, and no case has one that ends before `now`."""
    c = case(key)
    ev, sets = case_events(key, shifts), sets_of(key, shifts)
    now, hz = now_of(c.T), horizons_of(c.T)
    counts, accepted = expected(key, shifts)
    tot = accepted.sum(1).astype(np.int64)
    assert counts.shape == (5, len(hz), 2, c.n) and accepted.shape == (5, len(c.cands)) and len(hz) == 3 and now + hz[-1] == c.T - 1
    assert 1 <= tot[0] <= 12 and 1 <= tot[1] <= 12 and tot[2] == 0 and 5 <= tot[3] <= 140 and tot[4] == c.sims * len(c.cands), tot
    assert (accepted[4] == c.sims).all() and accepted[0, 2] >= 1 and tot[1] <= tot[0] <= tot[3]
    assert (counts.sum(2).max(-1).astype(np.int64) <= tot[:, None]).all() and (counts[2] == 0).all()
    assert counts[4, :, 0].sum() > 0 and counts[4, :, 1].sum() > 0 and counts[0].sum() > 0
    early = late = 0
    for o, records in enumerate(sets):
        for j, (t_inf, t_rec) in enumerate(ev):
            ok = accepted_rows(t_inf, t_rec, records, c.T, now)
            assert np.array_equal(agree_now_by_counter(t_inf, t_rec, records, c.T, now) == len(records), ok)
            end = end_step(t_inf[ok], t_rec[ok], c.T)
            early += int((end < now).sum()); late += int(((end >= now) & (end < now + hz[-1])).sum())
    assert early == 0 and (late > 0) == (key == "everybody"), (key, early, late)
    print(f"{key} {shifts}: now {now} horizons {hz}, accepted per set {tot.tolist()} of {c.sims * len(c.cands)}, "
          f"accepted trajectories that end before the last horizon {late}")


# ---------------------------------------------------------------------------------------------------------------- lonely
LONELY_GAMMA, LONELY_RNG = 0.3, 97


@functools.lru_cache(maxsize=None)
def lonely(key):
    """The `lonely` run on a case's graph: nobody infected at the start, every contact probability 0, gamma 0.3, the candidates
    [hub, n - 1], the sets (e) and [(hub, 0, 2)]; sims so that about 8 of the 2 x sims trajectories never end"""
    from types import SimpleNamespace
    c = case(key)
    hub = int(np.argmax(np.diff(c.rp)))
    sims = int(np.ceil(4.0 / (1.0 - LONELY_GAMMA) ** (c.T - 1)))
    sets = (((hub, -(c.T + 3), 0),), ((hub, 0, 2),))
    return SimpleNamespace(key=key, base=c.base, n=c.n, rp=c.rp, ci=c.ci, T=c.T, cands=[hub, c.n - 1], sims=sims, sets=sets, now=now_of(c.T),
                           horizons=horizons_of(c.T), rng_seed=LONELY_RNG, gamma=LONELY_GAMMA)


@functools.lru_cache(maxsize=None)
def lonely_events(key):
    r = lonely(key)
    p = np.tile([1.0, 0.0, 0.0], (r.n, 1))
    ev = Q.events(r.n, r.rp, r.ci, p, r.cands, [0, 0], [np.zeros(len(r.ci))], [r.gamma], np.zeros(r.T, np.int32), r.sims, r.T, r.rng_seed)
    return [tuple(SC._frozen(a) for a in e) for e in ev]


@functools.lru_cache(maxsize=None)
def lonely_expected(key):
    r = lonely(key)
    return tuple(SC._frozen(x) for x in posterior_of(lonely_events(key), r.sets, r.T, r.now, r.horizons, r.n))


def lonely_live(key):
    """Some trajectories end before `now`, some between `now` and the last horizon, some never; nobody but the candidate is
    ever counted; the second set accepts exactly the hub's trajectories that have recovered by `now`"""
    r = lonely(key)
    ev = lonely_events(key)
    counts, accepted = lonely_expected(key)
    end = np.concatenate([end_step(t_inf, t_rec, r.T) for t_inf, t_rec in ev])
    before, between, never = int((end < r.now).sum()), int(((end >= r.now) & (end < r.now + r.horizons[-1])).sum()), int((end == r.T).sum())
    assert before > 0 and between > 0 and never > 0, (key, before, between, never)
    assert all((t_inf >= 0).sum(1).max() == 1 for t_inf, _ in ev)
    hub, last = r.cands
    others = np.ones(r.n, bool); others[[hub, last]] = False
    assert (counts[:, :, :, others] == 0).all() and (accepted[0] == r.sims).all()
    assert accepted[1, 1] == 0 and accepted[1, 0] == ((ev[0][1][:, hub] >= 0) & (ev[0][1][:, hub] <= r.now)).sum() > 0
    assert (counts[1, :, 1, hub] == accepted[1, 0]).all() and (counts[1, :, 0] == 0).all()
    assert (counts[0, :, :, hub].sum(-1) == r.sims).all() and (np.diff(counts[0, :, 1, hub].astype(np.int64)) >= 0).all()
    print(f"lonely {key}: sims {r.sims}, trajectories that end before now {before}, between now and the last horizon {between}, never {never}")


# ------------------------------------------------------------------------------------------------------- the exact chain
# tests/sir_timed_model.py's chain (the triangle with a pendant node, T = 8) and its sets D, F, G at five (set, now), horizons
# (0, 1, 3), PER CANDIDATE: the candidates share their coins, so a count summed over them is no binomial
CHAIN_RUNS = (("D", 1), ("F", 3), ("G", 2), ("D", 0), ("F", 4))
CHAIN_HORIZONS = (0, 1, 3)
CHAIN_SIMS = 20_000


def chain_posterior(records, now, horizons=CHAIN_HORIZONS):
    """(joint float64 [4, H, 2, 4], total float64 [4]): P(every record matched at age `now`, node v in I / R at step now + h | node
    c alone infected at step 0) and P(every record matched | c) -- `sir_timed_model.chain_table`'s forward filter over the 81
    states up to step `now`, the masked vector then propagated h more steps unmasked and marginalised per node"""
    states, M = TM.chain_matrix()
    code = np.asarray(states)                                       # [81, 4]
    N = Q.CHAIN_N
    joint, total = np.zeros((N, len(horizons), 2, N)), np.zeros(N)
    for c in range(N):
        if any(now + d < 0 and kind != 0 for _, d, kind in records):
            continue
        x = np.zeros(len(states))
        x[states.index(tuple(int(v == c) for v in range(N)))] = 1.0
        for m in range(now + 1):
            here = [(v, kind) for v, d, kind in records if now + d == m]
            if m > 0:
                allowed = np.ones_like(M, dtype=bool)
                for v, kind in here:
                    if kind == 3:
                        allowed &= (code[:, v] == 0)[:, None] & (code[:, v] != 0)[None, :]
                    if kind == 4:
                        allowed &= (code[:, v] == 1)[:, None] & (code[:, v] == 2)[None, :]
                x = x @ (M * allowed)
            elif any(kind == 4 or (kind == 3 and v != c) for v, kind in here):
                x[:] = 0.0
            for v, kind in here:
                if kind <= 2:
                    x = x * (code[:, v] == kind)
        total[c] = x.sum()
        done = 0
        for j, h in enumerate(horizons):
            for _ in range(h - done):
                x = x @ M
            done = h
            for v in range(N):
                joint[c, j, 0, v], joint[c, j, 1, v] = x[code[:, v] == 1].sum(), x[code[:, v] == 2].sum()
    return joint, total


@functools.lru_cache(maxsize=None)
def _chain_events(sims):
    return TM.chain_events(sims)


@functools.lru_cache(maxsize=None)
def chain_counts(name, now, sims=CHAIN_SIMS):
    """(counts uint64 [4, H, 2, 4], accepted uint64 [4]) of the model PER CANDIDATE for one set of the chain"""
    out = [posterior_of([e], [TM.CHAIN_SETS[name]], TM.CHAIN_T, now, CHAIN_HORIZONS, Q.CHAIN_N) for e in _chain_events(sims)]
    return SC._frozen(np.stack([c[0] for c, _ in out])), SC._frozen(np.stack([a[0, 0] for _, a in out]))


def check_chain(name, now, counts, accepted, sims=CHAIN_SIMS):
    """the comparison of the issue on per-candidate counts [4, H, 2, 4] and accepted [4]; returns (largest share of the bound,
    cells with P >= 0.01)"""
    joint, total = chain_posterior(TM.CHAIN_SETS[name], now)
    assert np.allclose(total, TM.chain_table(TM.CHAIN_SETS[name])[:, now], rtol=0, atol=1e-14)
    assert np.allclose(joint[:, 0].sum(1).max(-1) <= total + 1e-14, True)
    est = counts.astype(np.float64) / sims
    share = np.abs(est - joint) / Q.chain_bound(joint, sims)
    ashare = np.abs(accepted.astype(np.float64) / sims - total) / Q.chain_bound(total, sims)
    print(f"set {name} now {now}: P(accepted | c) = {np.round(total, 4).tolist()}, accepted {accepted.tolist()} of {sims}; largest share of the "
          f"bound {float(share.max()):.3f} (accepted: {float(ashare.max()):.3f}); cells with P >= 0.01: {int((joint >= 0.01).sum())}")
    assert (share <= 1.0).all() and (ashare <= 1.0).all()
    assert (counts[joint == 0.0] == 0).all() and (accepted[total == 0.0] == 0).all()
    return float(share.max()), int((joint >= 0.01).sum())
