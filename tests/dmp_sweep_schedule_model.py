"""The CPU model of source scores and outbreak sizes under a rate schedule (a helper, not a test): what
gnode.dmp.source_scores_schedule and outbreak_sizes_schedule mean, in numpy.

A sample is a candidate and a SHIFT: step t = 1 .. T-1 of its run is governed by phase[shift + t], so its marginals are
`dmp_schedule_model.dmp_sir_schedule`'s float32 ones under the row phase[shift : shift + T] (entry 0 of a row is never read).
The scores are tests/test_gpu_dmp_source_events.py's `five_logs` composition of those marginals from the one-hot start, summed
over a row's coded nodes in float64; the sizes are the value-weighted float64 column sums from the base start with the
candidate's triple replaced.  `observed_at=D` is the diagonal: entry tau is the sample (c, D - tau) read at t = tau; the runs
are full-length, so the phase row is continued past step D with step D's phase, which no entry of the diagonal reads.

Behind them the sanity case of the two test modules: a snapshot of the tree case drawn by the Monte-Carlo model under a
three-phase lockdown, whose true source the scheduled scores rank first and the constant-rate scores do not."""
import functools

import numpy as np

import schedule_cases
from dmp_schedule_model import dmp_sir_schedule
from sir_schedule_model import schedule_thresholds, sir_events_schedule
from test_gpu_dmp_source_events import five_logs


def sample_marginals(rp, ci, W, G, phase, shift, p0, T):
    """float32 [T, n, 3] of one sample: DMP from the start p0 [n, 3] under the phase row moved by `shift`"""
    row = np.asarray(phase)[shift:shift + T]
    assert shift >= 0 and row.shape[0] == T, "shift + T must not exceed the phase row"
    return dmp_sir_schedule(rp, ci, W, G, row, p0, T)


def one_hot(n, c):
    p = np.zeros((n, 3))
    p[:, 0] = 1.0
    if 0 <= c < n:
        p[c] = (0.0, 1.0, 0.0)
    return p


def scores(rp, ci, W, G, phase, cands, shifts, rows, T, floor=1e-30):
    """float64 [R, C, T]: row r's log-likelihood at step t of sample (cands[j], shifts[j])"""
    n, rows = len(rp) - 1, np.asarray(rows)
    out = np.stack([sample_marginals(rp, ci, W, G, phase, int(s), one_hot(n, int(c)), T) for c, s in zip(cands, shifts)])
    logs = five_logs(out, floor)                                    # [5, C, T, n]
    table = np.zeros((len(rows), len(cands), T))
    for r, row in enumerate(rows):
        for code in range(5):
            table[r] += logs[code][:, :, row == code].sum(-1)
    return table


def scores_observed_at(rp, ci, W, G, phase, cands, rows, T, D, floor=1e-30):
    """float64 [R, C, T]: entry [r, c, tau] is the sample (c, D - tau) at t = tau -- c started tau steps before calendar step D"""
    assert D >= T - 1 and len(phase) >= D + 1
    phase = np.concatenate([np.asarray(phase)[:D + 1], np.full(T - 1, phase[D])])     # past step D nothing is read: step D's phase
    ids, shifts = np.repeat(np.asarray(cands), T), np.tile(D - np.arange(T), len(cands))
    table = scores(rp, ci, W, G, phase, ids, shifts, rows, T, floor).reshape(len(rows), len(cands), T, T)
    return np.ascontiguousarray(np.diagonal(table, axis1=2, axis2=3))


def sizes(rp, ci, W, G, phase, init, cands, shifts, action, value, T):
    """float64 [C, T, 3]: sum over the nodes of value[k] * P^k_j(t) for sample (cands[j], shifts[j]); a candidate outside the
    graph changes nothing"""
    n = len(rp) - 1
    v = np.ones(n) if value is None else np.asarray(value, dtype=np.float32).astype(np.float64)
    out = np.zeros((len(cands), T, 3))
    for j, (c, s) in enumerate(zip(cands, shifts)):
        p0 = np.array(init, dtype=np.float64)
        if 0 <= int(c) < n:
            p0[int(c)] = (0.0, 1.0, 0.0) if action == "seed" else (0.0, 0.0, 1.0)
        m = sample_marginals(rp, ci, W, G, phase, int(s), p0, T).astype(np.float64)
        out[j] = (v[None, :, None] * m).sum(1)
    return out


def ranking(table, cands):
    """the candidates of a [C, T] table by their best score over time, descending (ties keep the table's order), and the scores"""
    best = np.asarray(table).max(1)
    order = np.argsort(-best, kind="stable")
    return [int(np.asarray(cands)[i]) for i in order], best[order]


# ------------------------------------------------------------------------------------------------------------- the sanity case
# schedule_cases.tree(): the 120-node tree, open / a quarter of the contacts / closed but for the certain entries.  The calendar:
# open up to step 6, a quarter of the contacts at steps 7 .. 9, closed from step 10 on; the outbreak starts at calendar step
# D - TAU from the one node SOURCE and is seen, every node's state, at calendar step D.
SANITY = dict(D=13, TAU=9, T=12, source=4, rng_seed=5)
SANITY_PHASE = np.asarray([0] * 7 + [1] * 3 + [2] * 4, dtype=np.int32)     # [D + 1]


@functools.lru_cache(maxsize=None)
def sanity_case():
    """(n, rp, ci, W, G, phase, snapshot [1, n] of codes 0 / 1 / 2): one trajectory of the Monte-Carlo model from SOURCE under
    the calendar's row from step D - TAU on, read TAU steps later"""
    s = SANITY
    n, rp, ci, W, G, _ = schedule_cases.tree()
    THR, TG = schedule_thresholds(W, G, len(ci), n)
    row = SANITY_PHASE[s["D"] - s["TAU"]:]
    t_inf, t_rec = sir_events_schedule(n, rp, ci, [s["source"]], THR, TG, row, 1, s["TAU"] + 1, s["rng_seed"])
    snapshot = ((t_inf >= 0).astype(np.int8) + (t_rec >= 0).astype(np.int8)).reshape(1, n)
    snapshot.setflags(write=False)
    return n, rp, ci, W, G, SANITY_PHASE, snapshot


@functools.lru_cache(maxsize=None)
def sanity_tables():
    """(candidates, scheduled [C, T], constant [C, T]): the model's scores of the snapshot with observed_at = D under the true
    schedule, and under phase 0's rates held constant"""
    s = SANITY
    n, rp, ci, W, G, phase, snapshot = sanity_case()
    cands = np.flatnonzero(snapshot[0] >= 1)
    scheduled = scores_observed_at(rp, ci, W, G, phase, cands, snapshot, s["T"], s["D"])[0]
    constant = scores(rp, ci, W[:1], G[:1], np.zeros(s["T"], dtype=np.int32), cands, np.zeros(len(cands), dtype=int), snapshot, s["T"])[0]
    for a in (cands, scheduled, constant):
        a.setflags(write=False)
    return cands, scheduled, constant
