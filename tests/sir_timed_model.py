"""The CPU model of the Monte-Carlo source scores from timed evidence (`gnode_sir_mc_philox_sweep_timed`,
`source_scores_timed_mc`) and its cases, stated once (a helper, not a test).  numpy only.

The trajectories are those of tests/sir_score_model.py (`events`, `case_events`): candidate c's node seeded in the drawn start,
the phase row read from the candidate's shift on.  An evidence set is a list of records (node v, offset d <= 0, kind).  For
"now" = t steps after the run began a record is read at model step m = t + d and is MATCHED when

  m < 0                     kind == 0                                     (before the outbreak everybody is susceptible)
  m >= 0, kind 0 / 1 / 2    v is S / I / R at step m                      (`sir_state_at`'s codes)
  m >= 0, kind 3            t_inf[v] == m                                 (it became infected AT that step)
  m >= 0, kind 4            t_rec[v] == m                                 (it recovered AT that step)

agree[t] counts the matched records of the set and k = (agree[t] * bins) // records in integers, so k == bins exactly when
every record is matched.  hist[o, c, t, k] counts the trajectories of candidate c whose age t fell into bin k of set o.
`hist_of` is that definition; `hist_by_differences` restates the kernels' difference array over t, clamping included.

The cases are those of tests/sir_sweep_model.py with three evidence sets each (`evidence`): (a) what about 8 sensors report at
now = T // 2 of trajectory 0 of candidate index 2, by the rule of `gnode.dmp.observations_from_events` (onset, removal, state);
(b) the same plus a record further back than T, a second record on one node and a sensor that is a candidate; (c) a set no
trajectory can satisfy (a node recovers before it is infected)."""
import functools
import itertools

import numpy as np

import sir_cases as SC
import sir_score_model as Q
import sir_sweep_model as S

MAXO = Q.MAXO                                                       # GN_SIR_SCORE_MAXO of the library as built by default
CELLS = 2048                                                        # GN_SIR_TIMED_CELLS of the library as built by default


def matched(t_inf, t_rec, record, T):
    """bool [sims, T]: is the record matched when "now" is t, by the definition"""
    v, d, kind = (int(x) for x in record)
    ti, tr = np.asarray(t_inf)[:, v].astype(np.int64)[:, None], np.asarray(t_rec)[:, v].astype(np.int64)[:, None]
    m = (np.arange(T, dtype=np.int64) + d)[None, :]
    inf, rec = (ti >= 0) & (ti <= m), (tr >= 0) & (tr <= m)
    at = [~inf, inf & ~rec, rec, ti == m, tr == m][kind]
    return np.where(m < 0, kind == 0, at)


def agree_of(t_inf, t_rec, records, T):
    """int64 [sims, T]: the matched records of one set"""
    return sum(matched(t_inf, t_rec, r, T).astype(np.int64) for r in records)


def hist_of(events, sets, bins, T):
    """uint64 [O, C, T, bins + 1] from the per-candidate events [(t_inf, t_rec)] and the evidence sets, by the definition"""
    hist = np.zeros((len(sets), len(events), T, bins + 1), dtype=np.uint64)
    for o, records in enumerate(sets):
        for j, (t_inf, t_rec) in enumerate(events):
            k = (agree_of(t_inf, t_rec, records, T) * bins) // len(records)
            for t in range(T):
                hist[o, j, t] = np.bincount(k[:, t], minlength=bins + 1).astype(np.uint64)
    return hist


def agree_by_differences(t_inf, t_rec, records, T):
    """int64 [sims, T], as the kernels count it: dif[0] = the records of kind 0; a node's infection at step `it` adds -1 (kind 0)
    or +1 (kinds 1 and 3) at it + back, back = min(-d, T), and for kind 3 -1 again one cell later; its recovery adds -1 (kind 1)
    or +1 (kinds 2 and 4) at it + back and for kind 4 -1 one cell later; cells >= T are dropped; agree = the prefix sum over t"""
    t_inf, t_rec = np.asarray(t_inf).astype(np.int64), np.asarray(t_rec).astype(np.int64)
    dif = np.zeros((t_inf.shape[0], T), dtype=np.int64)
    dif[:, 0] = sum(int(r[2]) == 0 for r in records)

    def add(rows, pos, d):
        keep = pos < T
        np.add.at(dif, (rows[keep], pos[keep]), d)

    for v, d, kind in records:
        back = min(-int(d), T)
        for when, deltas in ((t_inf[:, v], {0: -1, 1: +1, 3: +1}), (t_rec[:, v], {1: -1, 2: +1, 4: +1})):
            if kind in deltas:
                rows = np.flatnonzero(when >= 0)
                add(rows, when[rows] + back, deltas[kind])
                if kind == (3 if 0 in deltas else 4):
                    add(rows, when[rows] + back + 1, -1)
    return np.cumsum(dif, axis=1)


def hist_by_differences(events, sets, bins, T):
    """`hist_of` through `agree_by_differences`"""
    hist = np.zeros((len(sets), len(events), T, bins + 1), dtype=np.uint64)
    for o, records in enumerate(sets):
        for j, (t_inf, t_rec) in enumerate(events):
            k = (agree_by_differences(t_inf, t_rec, records, T) * bins) // len(records)
            for t in range(T):
                hist[o, j, t] = np.bincount(k[:, t], minlength=bins + 1).astype(np.uint64)
    return hist


def reports(t_inf, t_rec, now, sensors, what=("onset", "removal", "state")):
    """[(node, offset, kind)]: the rule of `gnode.dmp.observations_from_events`, restated (tests/test_sir_timed_host.py holds
    the two together)"""
    out = []
    for w in what:
        for k in sensors:
            infected, recovered = 0 <= t_inf[k] <= now, 0 <= t_rec[k] <= now
            if w == "onset":
                out.append((int(k), int(t_inf[k] - now), 3) if infected else (int(k), 0, 0))
            elif w == "removal":
                if recovered:
                    out.append((int(k), int(t_rec[k] - now), 4))
            else:
                out.append((int(k), 0, int(infected) + int(recovered)))
    return out


class Observations:
    """An evidence set as `source_scores_timed_mc` takes it -- .rows int8 [R, n], .row_offsets, .n -- packed as
    `gnode.dmp.timed_observations` packs (descending offsets; a node's j-th record of an offset in that offset's j-th row)"""

    def __init__(self, n, records):
        rows, offs = [], []
        for d in sorted({int(r[1]) for r in records}, reverse=True):
            first, seen = len(rows), {}
            for v, _, kind in (r for r in records if int(r[1]) == d):
                j = seen.get(v, 0)
                seen[v] = j + 1
                if first + j == len(rows):
                    rows.append(np.full(n, -1, dtype=np.int8))
                    offs.append(d)
                rows[first + j][v] = kind
        self.rows, self.row_offsets, self.n = np.stack(rows), np.asarray(offs, dtype=np.int64), int(n)


def records_of(obs):
    """[(node, offset, kind)] of an `Observations` (or a `TimedObservations`) in the order the library reads them: by row, then
    by node"""
    r, v = np.nonzero(obs.rows >= 0)
    return [(int(b), int(obs.row_offsets[a]), int(obs.rows[a, b])) for a, b in zip(r, v)]


# ----------------------------------------------------------------------------------------------------------------- cases
KEYS = S.KEYS
case = Q.case
case_events = Q.case_events
# what the GPU module runs: every case under mixed shifts and under none, both bin choices between them
RUNS = [(k, s) for k in KEYS for s in ("mixed", "zeros")]


@functools.lru_cache(maxsize=None)
def evidence(key, shifts):
    """((a), (b), (c)) of the module's text for the case under `shifts`, each a tuple of records.  The sensors of (a): the first
    three nodes susceptible at now, the first three recovered, and infected ones up to eight in all."""
    c = case(key)
    t_inf, t_rec = (x[0] for x in case_events(key, shifts)[2])
    now = c.T // 2
    st = Q.states_at(t_inf[None, :], t_rec[None, :], now)[0]
    sus, inf, rec = (np.flatnonzero(st == k) for k in range(3))
    sensors = sus[:3].tolist() + rec[:3].tolist()
    sensors = sorted(sensors + inf[:8 - len(sensors)].tolist())
    a = reports(t_inf, t_rec, now, sensors)
    kinds = {r[2] for r in a}
    if key == "everybody":
        # nobody recovers before the switch step, which lies behind T // 2, and by then nobody is susceptible: no single "now"
        # of this case holds all three states, so the rule cannot give kinds 2 and 4 here; (b) and (c) bring them
        assert rec.size == 0 and kinds == {0, 1, 3}
    else:
        assert kinds == {0, 1, 2, 3, 4}, (key, kinds)
    first_i, cand = int(inf[0]), int(c.cands[2])
    b = a + [(sensors[0], -(c.T + 3), 0),                            # further back than T: before every outbreak, always matched
             (first_i, -1, int(0 <= t_inf[first_i] <= now - 1) + int(0 <= t_rec[first_i] <= now - 1)),     # a second (third) record on one node
             (cand, 0, int(st[cand])), (cand, -now, 3)]              # a sensor that is a candidate: its state, and its onset at step 0
    late = int(np.flatnonzero(t_rec >= 0)[-1])                       # a node that recovers at some step of this trajectory
    other = int(np.flatnonzero(t_rec >= 0)[0])
    cset = [(late, -2, 4), (late, 0, 3), (other, 0, 2), (other, -1, 4), (sensors[0], 0, 0)]
    assert {r[2] for r in b} | {r[2] for r in cset} == {0, 1, 2, 3, 4} and t_inf[cand] == 0
    assert first_i in sensors and sum(r[0] == first_i for r in b) >= 3 and cand in c.cands
    return tuple(a), tuple(b), tuple(cset)


def bins_of(key, shifts, bins):
    """bins = None is the library's default: the largest record count of the sets"""
    return max(len(s) for s in evidence(key, shifts)) if bins is None else bins


@functools.lru_cache(maxsize=None)
def expected(key, shifts, bins=None, sims=None, sim_offset=0):
    """hist of the model for a case against its three evidence sets, read-only"""
    c = case(key)
    return SC._frozen(hist_of(case_events(key, shifts, sims, sim_offset), evidence(key, shifts), bins_of(key, shifts, bins), c.T))


def live(key, shifts, bins=None):
    """On the model's own output: every (o, c, t) holds sims trajectories; the trajectory that made (a) and (b) is in their top
    bin at candidate index 2, now = T // 2; (c) has an empty top bin everywhere but matches some of its records somewhere; the
    record further back than T is matched at every t; and the difference-array form gives the same histogram."""
    c = case(key)
    ev, sets, B = case_events(key, shifts), evidence(key, shifts), bins_of(key, shifts, bins)
    h = expected(key, shifts, bins)
    assert h.shape == (3, len(c.cands), c.T, B + 1) and (h.sum(-1) == c.sims).all()
    assert h[0, 2, c.T // 2, B] >= 1 and h[1, 2, c.T // 2, B] >= 1
    assert (h[2, :, :, B] == 0).all() and h[2, :, :, 1:B].sum() > 0
    assert matched(ev[0][0], ev[0][1], sets[1][len(sets[0])], c.T).all() and -sets[1][len(sets[0])][1] >= c.T
    assert np.array_equal(hist_by_differences(ev, sets, B, c.T), h)
    print(f"{key} {shifts} bins {B}: records {[len(s) for s in sets]}, top-bin counts of (a) per candidate at T // 2 "
          f"{h[0, :, c.T // 2, B].tolist()} of {c.sims}")


# ------------------------------------------------------------------------------------------------------- the exact chain
# tests/sir_score_model.py's triangle 0-1-2 with the pendant node 3 on node 2, every contact w = 0.4, gamma = 0.3, every node a
# candidate from an all-susceptible start, T = 8; three evidence sets that use all five kinds between them
CHAIN_T = 8
CHAIN_SETS = {"D": ((3, 0, 0), (2, 0, 1), (0, -1, 1)), "F": ((0, 0, 2), (1, -1, 1), (3, 0, 0)), "G": ((2, -2, 3), (2, 0, 4), (3, 0, 0))}


@functools.lru_cache(maxsize=None)
def chain_matrix():
    """(states, float64 [81, 81]): on the pre-step state, a susceptible node with k infected neighbours is infected with
    probability 1 - (1 - w)^k and an infected node recovers with probability gamma, independently"""
    n, w, gamma = Q.CHAIN_N, Q.CHAIN_W, Q.CHAIN_GAMMA
    nb = [[] for _ in range(n)]
    for u, v in Q.CHAIN_EDGES:
        nb[u].append(v); nb[v].append(u)
    states = list(itertools.product(range(3), repeat=n))
    index = {s: i for i, s in enumerate(states)}
    M = np.zeros((len(states), len(states)))
    for s in states:
        per_node = []
        for v in range(n):
            if s[v] == 0:
                q = 1.0 - (1.0 - w) ** sum(s[u] == 1 for u in nb[v])
                per_node.append([(0, 1.0 - q), (1, q)])
            elif s[v] == 1:
                per_node.append([(1, 1.0 - gamma), (2, gamma)])
            else:
                per_node.append([(2, 1.0)])
        for combo in itertools.product(*per_node):
            M[index[s], index[tuple(x for x, _ in combo)]] += np.prod([p for _, p in combo])
    assert np.allclose(M.sum(1), 1.0, rtol=0, atol=1e-15)
    return states, M


def chain_table(records, T=CHAIN_T):
    """float64 [4, T]: P(every record matched | node c alone infected at step 0, now = t), by a forward filter over the 81
    states: at model step m the records read there mask states (kinds 0 to 2) and transitions into step m (kind 3: S to not-S,
    kind 4: I to R); at m = 0 kind 3 holds only for the candidate and kind 4 never; a record read before the outbreak holds
    iff its kind is 0"""
    states, M = chain_matrix()
    code = np.asarray(states)                                       # [81, 4]
    P = np.zeros((Q.CHAIN_N, T))
    for c in range(Q.CHAIN_N):
        for t in range(T):
            if any(t + d < 0 and kind != 0 for _, d, kind in records):
                continue
            x = np.zeros(len(states))
            x[states.index(tuple(int(v == c) for v in range(Q.CHAIN_N)))] = 1.0
            for m in range(t + 1):
                here = [(v, kind) for v, d, kind in records if t + d == m]
                if m > 0:
                    allowed = np.ones_like(M, dtype=bool)
                    for v, kind in here:
                        if kind == 3:
                            allowed &= (code[:, v] == 0)[:, None] & (code[:, v] != 0)[None, :]
                        if kind == 4:
                            allowed &= (code[:, v] == 1)[:, None] & (code[:, v] == 2)[None, :]
                    x = x @ (M * allowed)
                else:
                    if any(kind == 4 or (kind == 3 and v != c) for v, kind in here):
                        x[:] = 0.0
                for v, kind in here:
                    if kind <= 2:
                        x = x * (code[:, v] == kind)
            P[c, t] = x.sum()
    return P


def chain_events(sims, rng_seed=Q.CHAIN_RNG):
    rp, ci = Q.chain_csr()
    p = np.tile([1.0, 0.0, 0.0], (Q.CHAIN_N, 1))
    return Q.events(Q.CHAIN_N, rp, ci, p, list(range(Q.CHAIN_N)), [0] * Q.CHAIN_N, [np.full(len(ci), Q.CHAIN_W)], [Q.CHAIN_GAMMA],
                    np.zeros(CHAIN_T, np.int32), sims, CHAIN_T, rng_seed)


def chain_hist(sims, rng_seed=Q.CHAIN_RNG):
    """uint64 [3, 4, T, 4]: the model's histogram of the sets D, F, G (three records each, bins = 3), candidates 0 .. 3"""
    return hist_of(chain_events(sims, rng_seed), [CHAIN_SETS[k] for k in "DFG"], 3, CHAIN_T)


def check_chain(hist, sims):
    """the comparison of the issue, on a histogram uint64 [3, 4, T, 4] of the sets D, F, G"""
    total = 0
    for o, name in enumerate("DFG"):
        P = chain_table(CHAIN_SETS[name])
        est = hist[o, :, :, 3].astype(np.float64) / sims
        share = np.abs(est - P) / Q.chain_bound(P, sims)
        print(f"set {name}: P =", np.round(P, 4).tolist())
        print(f"set {name}: estimate =", np.round(est, 4).tolist())
        print(f"set {name}: largest share of the bound:", float(share.max()), "at", np.unravel_index(share.argmax(), share.shape),
              "cells with P >= 0.01:", int((P >= 0.01).sum()))
        assert (hist[o].sum(-1) == sims).all()
        assert (share <= 1.0).all()
        assert (hist[o, :, :, 3][P == 0.0] == 0).all()
        assert np.unravel_index(est.argmax(), est.shape) == np.unravel_index(P.argmax(), P.shape)
        total += int((P >= 0.01).sum())
    assert total >= 30
