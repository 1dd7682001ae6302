"""The CPU model of the Monte-Carlo nowcast from evidence that may be wrong (`gnode_sir_mc_philox_sweep_posterior_strata`,
`posterior_strata_mc`) and its cases, stated once (a helper, not a test).  numpy only.

The trajectories, the records and `now` are those of tests/sir_post_model.py.  For trajectory (c, s) and an evidence set,
d = len(records) - agree_of(...)[s, now] is the number of records it MISSES; with M = mismatches it is accepted for the set in
STRATUM d iff d <= M.  accepted[o, c, d] counts the trajectories of candidate c in stratum d; counts[o, d, j, 0, v] counts, over
the trajectories of ALL candidates in stratum d, those in which node v is I at step now + horizons[j], and counts[o, d, j, 1, v]
those in which it is R (`states_at`: a trajectory that ended early keeps its final state).  `strata_of` is that definition;
`strata_by_counter` restates the kernels' reading, records - the one counter per set of tests/sir_post_model.py.

The cases are those of tests/sir_post_model.py (`RUNS`, `now_of`, `horizons_of`) at M = 2 with eight evidence sets
(`sets_of`): that module's (a) to (e); (d1) = (d) plus one record that nothing matches -- kind 1, "infected", read before the
outbreak; (e2) = (e) plus two of them; (e3) = (e) plus three.  The `lonely` runs take their two sets and the hub's (e) with one
never-matched record, at M = 1.  The exact chain is `chain_strata`: tests/sir_post_model.py's forward filter with a mismatch
counter."""
import functools

import numpy as np

import sir_cases as SC
import sir_post_model as PM
import sir_score_model as Q
import sir_timed_model as TM

MAXD = 8                                                            # GN_SIR_POST_MAXD of the library as built by default
M_CASES, M_LONELY = 2, 1


def missed_of(t_inf, t_rec, records, T, now):
    """int64 [sims]: the records of the set that are NOT matched at age `now`, by the definition"""
    return len(records) - TM.agree_of(t_inf, t_rec, records, T)[:, now]


def strata_of(events, sets, T, now, horizons, n, M):
    """(counts uint64 [O, D, H, 2, n], accepted uint64 [O, C, D]), D = M + 1, from the per-candidate events [(t_inf, t_rec)], by
    the definition"""
    D = M + 1
    counts = np.zeros((len(sets), D, len(horizons), 2, n), dtype=np.uint64)
    accepted = np.zeros((len(sets), len(events), D), dtype=np.uint64)
    for o, records in enumerate(sets):
        for c, (t_inf, t_rec) in enumerate(events):
            miss = missed_of(t_inf, t_rec, records, T, now)
            for d in range(D):
                ok = miss == d
                accepted[o, c, d] = ok.sum()
                for j, h in enumerate(horizons):
                    st = Q.states_at(t_inf[ok], t_rec[ok], now + int(h))
                    counts[o, d, j, 0] += (st == 1).sum(0).astype(np.uint64)
                    counts[o, d, j, 1] += (st == 2).sum(0).astype(np.uint64)
    return counts, accepted


def strata_by_counter(t_inf, t_rec, records, T, now):
    """int64 [sims], as the kernels read it: records - the counter that moved with the events up to step `now`"""
    return len(records) - PM.agree_now_by_counter(t_inf, t_rec, records, T, now)


# ----------------------------------------------------------------------------------------------------------------- cases
KEYS, RUNS = PM.KEYS, PM.RUNS
case, case_events, now_of, horizons_of = PM.case, PM.case_events, PM.now_of, PM.horizons_of
A, B, C, D, E, D1, E2, E3 = range(8)                               # the sets' places in sets_of


@functools.lru_cache(maxsize=None)
def sets_of(key, shifts):
    """((a), (b), (c), (d), (e), (d1), (e2), (e3)) of the module's text"""
    c = case(key)
    a, b, cset, d, e = PM.sets_of(key, shifts)
    never = (a[0][0], -(c.T + 3), 1)
    return a, b, cset, d, e, d + (never,), e + (never,) * 2, e + (never,) * 3


@functools.lru_cache(maxsize=None)
def expected(key, shifts, M=M_CASES, sims=None, sim_offset=0):
    """(counts, accepted) of the model for a case against its eight sets, read-only"""
    c = case(key)
    out = strata_of(case_events(key, shifts, sims, sim_offset), sets_of(key, shifts), c.T, now_of(c.T), horizons_of(c.T), c.n, M)
    return tuple(SC._frozen(x) for x in out)


# the accepted trajectories of (d) by stratum, all candidates, as a probe of this model found them when the cases were chosen
PROBED_D = {"er-small/init": ([83, 117, 0], [140, 60, 0]), "hubs/init": ([20, 40, 0],), "large/init": ([5, 19, 0], [6, 18, 0]),
            "global-lists/init": ([45, 0, 0],)}


def live(key, shifts):
    """On the model's own output: stratum 0 is tests/sir_post_model.py's posterior; (d) has two records, so its strata 0 and 1
    hold every trajectory -- the probed numbers -- and (d1) is (d) moved by one stratum; (e2) holds every trajectory in stratum 2
    and (e3) accepts nothing; every stratum 0, 1, 2 is non-empty for some set; no count exceeds its stratum's total; the counter
    form gives the same strata."""
    c = case(key)
    ev, sets = case_events(key, shifts), sets_of(key, shifts)
    now, hz = now_of(c.T), horizons_of(c.T)
    counts, accepted = expected(key, shifts)
    post_counts, post_accepted = PM.expected(key, shifts)
    everyone = c.sims * len(c.cands)
    by = accepted.sum(1).astype(np.int64)                           # [8, 3]
    assert counts.shape == (8, 3, len(hz), 2, c.n) and accepted.shape == (8, len(c.cands), 3)
    assert np.array_equal(counts[:5, 0], post_counts) and np.array_equal(accepted[:5, :, 0], post_accepted)
    assert by[D, 2] == 0 and by[D, 0] >= 1 and by[D, 0] + by[D, 1] == everyone, by[D]
    if key in PROBED_D:
        assert by[D].tolist() in [list(x) for x in PROBED_D[key]], (key, shifts, by[D])
    assert by[D1].tolist() == [0, by[D, 0], by[D, 1]]
    assert np.array_equal(accepted[D1, :, 1:], accepted[D, :, :2]) and np.array_equal(counts[D1, 1:], counts[D, :2]) and (counts[D1, 0] == 0).all()
    assert by[E].tolist() == [everyone, 0, 0] and by[E2].tolist() == [0, 0, everyone] and (accepted[E2, :, 2] == c.sims).all()
    assert np.array_equal(counts[E2, 2], counts[E, 0]) and (by[E3] == 0).all() and (counts[E3] == 0).all()
    assert ((by > 0).any(0)).all()
    assert (counts.sum(3).max(-1).astype(np.int64) <= by[:, :, None]).all()
    for records in sets:
        for t_inf, t_rec in ev:
            assert np.array_equal(strata_by_counter(t_inf, t_rec, records, c.T, now), missed_of(t_inf, t_rec, records, c.T, now))
    print(f"{key} {shifts}: now {now} horizons {hz}, accepted by stratum per set {by.tolist()} of {everyone}")


# ---------------------------------------------------------------------------------------------------------------- lonely
@functools.lru_cache(maxsize=None)
def lonely_sets(key):
    """the two sets of tests/sir_post_model.py's `lonely` run and the hub's always-matched record with one that nothing matches"""
    r = PM.lonely(key)
    hub = r.cands[0]
    return r.sets + (((hub, -(r.T + 3), 0), (hub, -(r.T + 3), 1)),)


@functools.lru_cache(maxsize=None)
def lonely_expected(key):
    r = PM.lonely(key)
    return tuple(SC._frozen(x) for x in strata_of(PM.lonely_events(key), lonely_sets(key), r.T, r.now, r.horizons, r.n, M_LONELY))


def lonely_live(key):
    """tests/sir_post_model.py's `lonely_live` (ends before `now`, between the horizons, never) holds for the run; stratum 0 of
    its two sets is its output, their stratum 1 holds what is left, and the third set holds everything in stratum 1"""
    PM.lonely_live(key)
    r = PM.lonely(key)
    counts, accepted = lonely_expected(key)
    post_counts, post_accepted = PM.lonely_expected(key)
    assert np.array_equal(counts[:2, 0], post_counts) and np.array_equal(accepted[:2, :, 0], post_accepted)
    assert (accepted[:2].sum(-1) == r.sims).all() and accepted[1, :, 1].sum() > 0           # one record each: d is 0 or 1
    assert (accepted[2, :, 0] == 0).all() and (accepted[2, :, 1] == r.sims).all() and np.array_equal(counts[2, 1], counts[0, 0])


# ------------------------------------------------------------------------------------------------------- the exact chain
CHAIN_RUNS, CHAIN_HORIZONS, CHAIN_SIMS, CHAIN_M = PM.CHAIN_RUNS, PM.CHAIN_HORIZONS, PM.CHAIN_SIMS, 3


def _moved(X, k):
    """the mass of every stratum d moved to d + k (what would pass the last row is dropped: the rows cover every record)"""
    if k == 0:
        return X
    out = np.zeros_like(X)
    out[k:] = X[:X.shape[0] - k]
    return out


def chain_strata(records, now, M, horizons=CHAIN_HORIZONS):
    """(joint float64 [4, D, H, 2, 4], total float64 [4, D]), D = M + 1: P(exactly d records missed at age `now`, node v in I / R
    at step now + h | node c alone infected at step 0) and P(exactly d missed | c).  `sir_post_model.chain_posterior`'s forward
    filter over the 81 states with the vector widened to [R + 1, 81], one row per number of records missed so far: a state
    record (kinds 0 to 2) that is not matched moves the mass of its states from row d to d + 1 instead of masking it; a step
    with k unmatched transition records (kinds 3 / 4) moves the mass of that transition by k; a record read before the outbreak
    moves everything by one unless its kind is 0; at m = 0 kind 3 holds for the candidate only and kind 4 never."""
    states, P = TM.chain_matrix()
    code = np.asarray(states)                                       # [81, 4]
    N, R, D = Q.CHAIN_N, len(records), M + 1
    joint, total = np.zeros((N, D, len(horizons), 2, N)), np.zeros((N, D))
    for c in range(N):
        X = np.zeros((max(R, M) + 1, len(states)))
        X[0, states.index(tuple(int(v == c) for v in range(N)))] = 1.0
        X = _moved(X, sum(now + d < 0 and kind != 0 for _, d, kind in records))
        for m in range(now + 1):
            here = [(v, kind) for v, d, kind in records if now + d == m]
            if m > 0:
                miss = np.zeros(P.shape, dtype=np.int64)            # per transition: its unmatched transition records
                for v, kind in here:
                    if kind == 3:
                        miss += ~((code[:, v] == 0)[:, None] & (code[:, v] != 0)[None, :])
                    if kind == 4:
                        miss += ~((code[:, v] == 1)[:, None] & (code[:, v] == 2)[None, :])
                X = sum(_moved(X @ (P * (miss == k)), k) for k in range(int(miss.max()) + 1))
            else:
                X = _moved(X, sum(kind == 4 or (kind == 3 and v != c) for v, kind in here))
            for v, kind in here:
                if kind <= 2:
                    ok = code[:, v] == kind
                    X = X * ok + _moved(X * ~ok, 1)
        total[c] = X[:D].sum(1)
        done = 0
        for j, h in enumerate(horizons):
            for _ in range(h - done):
                X = X @ P
            done = h
            for v in range(N):
                joint[c, :, j, 0, v], joint[c, :, j, 1, v] = X[:D, code[:, v] == 1].sum(1), X[:D, code[:, v] == 2].sum(1)
    return joint, total


@functools.lru_cache(maxsize=None)
def chain_counts(name, now, M=CHAIN_M, sims=CHAIN_SIMS):
    """(counts uint64 [4, D, H, 2, 4], accepted uint64 [4, D]) of the model PER CANDIDATE for one set of the chain"""
    out = [strata_of([e], [TM.CHAIN_SETS[name]], TM.CHAIN_T, now, CHAIN_HORIZONS, Q.CHAIN_N, M) for e in PM._chain_events(sims)]
    return SC._frozen(np.stack([c[0] for c, _ in out])), SC._frozen(np.stack([a[0, 0] for _, a in out]))


def check_chain(name, now, counts, accepted, M=CHAIN_M, sims=CHAIN_SIMS):
    """the comparison of the issue on per-candidate counts [4, D, H, 2, 4] and accepted [4, D]: every cell of counts / sims and
    accepted / sims within `chain_bound` of the filter's probability, zero where that is zero; returns (largest share of the
    bound, cells with P >= 0.01)"""
    joint, total = chain_strata(TM.CHAIN_SETS[name], now, M)
    share = np.abs(counts.astype(np.float64) / sims - joint) / Q.chain_bound(joint, sims)
    ashare = np.abs(accepted.astype(np.float64) / sims - total) / Q.chain_bound(total, sims)
    print(f"set {name} now {now}: P(d missed | c) = {np.round(total, 4).tolist()}, accepted {accepted.tolist()} of {sims}; largest share of the "
          f"bound {float(share.max()):.3f} (accepted: {float(ashare.max()):.3f}); cells with P >= 0.01: {int((joint >= 0.01).sum())}")
    assert (share <= 1.0).all() and (ashare <= 1.0).all()
    assert (counts[joint == 0.0] == 0).all() and (accepted[total == 0.0] == 0).all()
    return float(max(share.max(), ashare.max())), int((joint >= 0.01).sum())
