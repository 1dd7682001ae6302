"""CPU model of the Monte-Carlo SIR labels with per-edge transmission probabilities (a helper, not a test).

The loop of tests/sir_nodes_model.py with the infection threshold taken at the CSR position: the directed entry at
position p, in row u with col[p] = v, fires iff coin(p, step, sim) < thr(w[p]) -- w[p] is the probability that u (the row)
infects v (the column).  Recovery is per node.  Coins and thresholds are the oracle's; tests/test_sir_edges_model.py holds
this helper to `sir_philox` and to the per-node model.  `return_events=True` also returns the step at which each node of
each trajectory left S and the step at which it recovered (-1: never), which the counts fold away."""
import numpy as np

from gnode_oracle import coin_threshold, philox_coin
from sir_nodes_model import thresholds


def sir_philox_edges(n, rowptr, col, seed_set, w, gamma, sims, T, rng_seed, sim_offset=0, return_events=False):
    """uint32 counts [3, T, n] (S, I, R), row-0 quirk included, for w[p] per CSR position and gamma[u] per node (a scalar
    broadcasts); with return_events also int16 t_inf, t_rec [sims, n]."""
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    dst = np.asarray(col).astype(np.int64)
    nnz = dst.shape[0]
    eid = np.arange(nnz, dtype=np.uint64)
    k0, k1 = np.uint64(rng_seed & 0xFFFFFFFF), np.uint64((rng_seed >> 32) & 0xFFFFFFFF)
    tw = np.asarray([coin_threshold(x) for x in np.broadcast_to(np.asarray(w, dtype=np.float64), (nnz,))], dtype=np.uint64)
    tg = thresholds(gamma, n)
    cnt = np.zeros((3, T, n), dtype=np.uint32)
    t_inf = np.full((sims, n), -1, dtype=np.int16)
    t_rec = np.full((sims, n), -1, dtype=np.int16)
    for k, s in enumerate(range(sim_offset, sim_offset + sims)):
        I = np.zeros(n, dtype=bool); S = np.ones(n, dtype=bool); R = np.zeros(n, dtype=bool)
        I[list(seed_set)] = True; S[list(seed_set)] = False
        t_inf[k, list(seed_set)] = 0
        cnt[0, 0] = S; cnt[1, 0] = I
        for it in range(1, T):
            act = np.nonzero(I[src] & S[dst])[0]
            c = philox_coin(eid[act], it, s, 0, k0, k1)
            new_inf = dst[act[c < tw[act]]]
            idx_I = np.nonzero(I)[0]
            c2 = philox_coin(idx_I.astype(np.uint64), it, s, 1, k0, k1)
            new_rec = idx_I[c2 < tg[idx_I]]
            R[new_rec] = True
            I[new_inf] = True; I[new_rec] = False; S[new_inf] = False
            t_inf[k, new_inf] = it
            t_rec[k, new_rec] = it
            cnt[0, it] += S; cnt[1, it] += I; cnt[2, it] += R
    return (cnt, t_inf, t_rec) if return_events else cnt


def one_way_path(k):
    """(n, rowptr, col, w) of the line 0 - 1 - ... - k with w = 1 on every entry i -> i + 1 and 0 on every i + 1 -> i."""
    n = k + 1
    rows = [[j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.asarray([j for r in rows for j in r], dtype=np.int32)
    src = np.repeat(np.arange(n), np.diff(rowptr))
    return n, rowptr, col, (col > src).astype(np.float64)
