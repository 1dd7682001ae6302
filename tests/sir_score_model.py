"""The CPU model of the Monte-Carlo source scores (`gnode_sir_mc_philox_sweep_scores`, `source_scores_mc`) and its cases, stated
once (a helper, not a test).  numpy only.

The model: for each candidate c, `sir_schedule_model.sir_events_schedule` from the start p whose row c is replaced by (0, 1, 0)
(an id outside [0, n) replaces nothing), under the phase row taken from the candidate's shift on -- exactly what
`sir_sweep_model.sweep` simulates.  The state of every trajectory at every step t is read off (t_inf, t_rec), and its
similarity with each snapshot (int8 [n], -1 not observed, 0 / 1 / 2 = S / I / R) is computed by its SET definition:

  "jaccard"  A = {v : obs[v] in {1, 2}},  B = {v : obs[v] >= 0 and state[v] != S}:   num = |A & B|, den = |A | B|
  "match"    num = |{v : obs[v] >= 0 and obs[v] == state[v]}|,                        den = |{v : obs[v] >= 0}|

The bin is k = (num * bins) // den in integers, k = bins when den = 0, so k = bins exactly when the two agree completely.
hist[o, c, t, k] counts the trajectories of candidate c whose step t fell into bin k of snapshot o.

The cases are those of tests/sir_sweep_model.py (shapes, candidates, mixed shifts, sims) with three snapshots each:
(a) the state at step T // 2 of trajectory 0 of candidate index 2, fully observed; (b) the same with every third node not
observed; (c) a snapshot holding all three codes that no trajectory produced."""
import functools

import numpy as np

import sir_cases as SC
import sir_sweep_model as S
from sir_schedule_model import schedule_thresholds, sir_events_schedule

MEASURES = {"jaccard": 0, "match": 1}
MAXO = 16                                                           # GN_SIR_SCORE_MAXO of the library as built by default


def states_at(t_inf, t_rec, t):
    """int8 [sims, n]: 0 S, 1 I, 2 R at step t (`gnode.ode_nn.sir_state_at`)"""
    return (((t_inf >= 0) & (t_inf <= t)).astype(np.int8) + ((t_rec >= 0) & (t_rec <= t)).astype(np.int8))


def bin_of(num, den, bins):
    """int64: (num * bins) // den, and `bins` where den = 0"""
    num, den = np.asarray(num, dtype=np.int64), np.asarray(den, dtype=np.int64)
    return np.where(den == 0, bins, (num * bins) // np.maximum(den, 1))


def similarity_bins(state, obs, measure, bins):
    """int64 [O, sims]: the bin of every trajectory's state (int8 [sims, n]) against every snapshot (int8 [O, n])"""
    out = np.empty((obs.shape[0], state.shape[0]), dtype=np.int64)
    for o, ob in enumerate(obs):
        seen = ob >= 0
        if measure == "jaccard":
            A, B = (ob >= 1)[None, :], seen[None, :] & (state != 0)
            num, den = (A & B).sum(1), (A | B).sum(1)
        else:
            num, den = (seen[None, :] & (state == ob[None, :])).sum(1), np.full(state.shape[0], int(seen.sum()))
        out[o] = bin_of(num, den, bins)
    return out


def hist_of(events, obs, measure, bins, T):
    """uint64 [O, C, T, bins + 1] from the per-candidate events [(t_inf, t_rec)]"""
    obs = np.atleast_2d(np.asarray(obs, dtype=np.int8))
    hist = np.zeros((obs.shape[0], len(events), T, bins + 1), dtype=np.uint64)
    for j, (t_inf, t_rec) in enumerate(events):
        for t in range(T):
            k = similarity_bins(states_at(t_inf, t_rec, t), obs, measure, bins)
            for o in range(obs.shape[0]):
                hist[o, j, t] = np.bincount(k[o], minlength=bins + 1).astype(np.uint64)
    return hist


def events(n, rp, ci, p, cands, shifts, W, G, phase, sims, T, rng_seed, sim_offset=0, thresholds=None):
    """[(t_inf, t_rec)] per candidate: the trajectories `sir_sweep_model.sweep` sums, kept"""
    THR, TG = thresholds or schedule_thresholds(W, G, len(ci), n)
    phase = np.asarray(phase)
    done, out = {}, []
    for c, k in zip(cands, shifts):
        c, k = int(c), int(k)
        if (c, k) not in done:
            q = np.array(p, dtype=np.float64)
            if 0 <= c < n:
                q[c] = S.ROW["seed"]
            assert k >= 0 and k + T <= len(phase)
            done[(c, k)] = sir_events_schedule(n, rp, ci, q, THR, TG, phase[k:], sims, T, rng_seed, sim_offset)
        out.append(done[(c, k)])
    return out


def scores(n, rp, ci, p, cands, shifts, W, G, phase, obs, measure, bins, sims, T, rng_seed, sim_offset=0):
    """uint64 [O, C, T, bins + 1] of the model"""
    return hist_of(events(n, rp, ci, p, cands, shifts, W, G, phase, sims, T, rng_seed, sim_offset), obs, measure, bins, T)


def kernel_scores(hist, sims, width=0.25, floor=1e-30):
    """float64 [..., C, T]: log(max(floor, sum_k hist[..., k] exp(-(1 - k / bins)^2 / width^2) / sims)), a bin at its lower edge"""
    bins = hist.shape[-1] - 1
    wgt = np.exp(-(1.0 - np.arange(bins + 1, dtype=np.float64) / bins) ** 2 / width ** 2)
    return np.log(np.maximum(floor, (hist.astype(np.float64) * wgt).sum(-1) / sims))


# ----------------------------------------------------------------------------------------------------------------- cases
KEYS = S.KEYS
case = S.case
# what the GPU module runs: every case under both measures, both bin counts and both shift rows between its two runs; er-small
# under all eight
RUNS = [(k, m, b, s) for k in KEYS for m, b, s in (("jaccard", 64, "mixed"), ("match", 7, "zeros"))] + \
       [("er-small/init", m, b, s) for m in MEASURES for b in (64, 7) for s in ("mixed", "zeros")
        if (m, b, s) not in (("jaccard", 64, "mixed"), ("match", 7, "zeros"))]


@functools.lru_cache(maxsize=None)
def case_events(key, shifts, sims=None, sim_offset=0):
    c = case(key)
    ev = events(c.n, c.rp, c.ci, c.p, c.cands, getattr(c, shifts), c.W, c.G, c.phase, c.sims if sims is None else sims, c.T, c.rng_seed,
                sim_offset, thresholds=S._thresholds(key))
    return [tuple(SC._frozen(a) for a in e) for e in ev]


@functools.lru_cache(maxsize=None)
def snapshots(key, shifts):
    """int8 [3, n], read-only: (a), (b), (c) of the module's text for the case under `shifts` ("mixed" or "zeros")"""
    c = case(key)
    t_inf, t_rec = case_events(key, shifts)[2]
    a = states_at(t_inf[:1], t_rec[:1], c.T // 2)[0]
    b = a.copy()
    b[::3] = -1
    odd = (np.arange(c.n) % 3).astype(np.int8)                     # S, I, R in rotation over the node ids
    return SC._frozen(np.stack([a, b, odd]))


@functools.lru_cache(maxsize=None)
def expected(key, measure, bins, shifts, sims=None, sim_offset=0):
    """hist of the model for a case against its three snapshots, read-only"""
    c = case(key)
    return SC._frozen(hist_of(case_events(key, shifts, sims, sim_offset), snapshots(key, shifts), measure, bins, c.T))


def live(key, measure, bins, shifts):
    """On the model's own output: every (o, c, t) holds sims trajectories; snapshot (a) puts its own trajectory into the top bin
    of candidate index 2 at step T // 2, and (b), which observes fewer nodes, at least as many; no trajectory of any candidate
    reaches the top bin of (c) at any step; the three snapshots give three different histograms; some trajectory lies in a bin
    strictly between 0 and the top."""
    c = case(key)
    h = expected(key, measure, bins, shifts)
    obs = snapshots(key, shifts)
    assert h.shape == (3, len(c.cands), c.T, bins + 1) and (h.sum(-1) == c.sims).all()
    assert h[0, 2, c.T // 2, bins] >= 1 and h[1, 2, c.T // 2, bins] >= h[0, 2, c.T // 2, bins]
    assert all((np.unique(obs[2]) == [0, 1, 2]).tolist()) and (h[2, :, :, bins] == 0).all()
    assert (obs[1] == -1).sum() == (c.n + 2) // 3 and (obs[0] >= 0).all()
    assert not np.array_equal(h[0], h[2]) and not np.array_equal(h[1], h[2])
    assert h[:, :, :, 1:bins].sum() > 0
    print(f"{key} {measure} {bins} {shifts}: top-bin counts of (a) per candidate at T // 2 {h[0, :, c.T // 2, bins].tolist()} of {c.sims}")


# ------------------------------------------------------------------------------------------------------- the exact chain
# The triangle 0-1-2 with the pendant node 3 on node 2, every contact w = 0.4, gamma = 0.3, T = 6, every node a candidate from
# an all-susceptible start; the snapshot (R, I, I, S), fully observed, under "match": the top bin is the exact-match frequency.
CHAIN_N, CHAIN_T, CHAIN_W, CHAIN_GAMMA, CHAIN_RNG = 4, 6, 0.4, 0.3, 2468
CHAIN_EDGES = [(0, 1), (0, 2), (1, 2), (2, 3)]
CHAIN_OBS = np.asarray([2, 1, 1, 0], dtype=np.int8)


def chain_csr():
    nb = [[] for _ in range(CHAIN_N)]
    for u, v in CHAIN_EDGES:
        nb[u].append(v); nb[v].append(u)
    rp = np.concatenate([[0], np.cumsum([len(x) for x in nb])]).astype(np.int64)
    return rp, np.asarray([v for x in nb for v in sorted(x)], dtype=np.int64)


def chain_hist(sims, bins=4, rng_seed=CHAIN_RNG):
    """uint64 [4, T, bins + 1]: the model's histogram of the chain's snapshot, candidates 0 .. 3"""
    rp, ci = chain_csr()
    p = np.tile([1.0, 0.0, 0.0], (CHAIN_N, 1))
    return scores(CHAIN_N, rp, ci, p, list(range(CHAIN_N)), [0] * CHAIN_N, [np.full(len(ci), CHAIN_W)], [CHAIN_GAMMA], np.zeros(CHAIN_T, np.int32),
                  CHAIN_OBS, "match", bins, sims, CHAIN_T, rng_seed)[0]


def chain_bound(P, sims):
    """5 sigma of a Bernoulli cell plus one count"""
    return 5.0 * np.sqrt(P * (1.0 - P) / sims) + 1.0 / sims
