"""CPU model of the per-trajectory Monte-Carlo SIR output (a helper, not a test).

The step loop of tests/sir_nodes_model.py::sir_philox_nodes, recording instead of accumulating: for the call's s-th trajectory
(coins of sim_offset + s) the step at which each node was infected (0 for a seed) and recovered, -1 for never within T,
and the population totals (S_t, I_t, R_t) of every step, row 0 the true initial state.  Coins and thresholds are the
oracle's (`philox_coin`, `coin_threshold`); tests/test_sir_events_model.py holds this helper to `sir_philox` and
`sir_philox_nodes`."""
import numpy as np

from gnode_oracle import philox_coin
from sir_nodes_model import thresholds


def sir_philox_events(n, rowptr, col, seed_set, beta, gamma, sims, T, rng_seed, sim_offset=0):
    """(t_inf int16 [sims, n], t_rec int16 [sims, n], curves uint32 [sims, T, 3]) for beta[v] / gamma[u] per node (a scalar
    broadcasts).  The step loop carries a block of trajectories at a time (state [block, n]; the coins take the
    trajectory id as an array), which is the per-trajectory loop with its Python overhead paid once per block."""
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    dst = col.astype(np.int64)
    eid = np.arange(col.shape[0], dtype=np.uint64)
    k0, k1 = np.uint64(rng_seed & 0xFFFFFFFF), np.uint64((rng_seed >> 32) & 0xFFFFFFFF)
    tb, tg = thresholds(beta, n), thresholds(gamma, n)
    t_inf = np.full((sims, n), -1, dtype=np.int16)
    t_rec = np.full((sims, n), -1, dtype=np.int16)
    curves = np.zeros((sims, T, 3), dtype=np.uint32)
    block = max(1, min(sims, (1 << 23) // max(int(col.shape[0]), n, 1)))
    for j0 in range(0, sims, block):
        m = min(block, sims - j0)
        sim = (sim_offset + j0 + np.arange(m)).astype(np.uint64)
        I = np.zeros((m, n), dtype=bool); S = np.ones((m, n), dtype=bool); R = np.zeros((m, n), dtype=bool)
        I[:, list(seed_set)] = True; S[:, list(seed_set)] = False
        t_inf[j0:j0 + m][I] = 0
        curves[j0:j0 + m, 0] = np.stack([S.sum(1), I.sum(1), R.sum(1)], axis=1)
        for it in range(1, T):
            aj, ae = np.nonzero(I[:, src] & S[:, dst])                 # (trajectory, CSR entry): infected source, susceptible target
            w = philox_coin(eid[ae], it, sim[aj], 0, k0, k1)
            fire = w < tb[dst[ae]]
            ij, iv = aj[fire], dst[ae[fire]]
            rj, ru = np.nonzero(I)                                     # both decided on the pre-step state
            w2 = philox_coin(ru.astype(np.uint64), it, sim[rj], 1, k0, k1)
            gone = w2 < tg[ru]
            rj, ru = rj[gone], ru[gone]
            t_inf[j0 + ij, iv] = it; t_rec[j0 + rj, ru] = it
            R[rj, ru] = True
            I[ij, iv] = True; I[rj, ru] = False; S[ij, iv] = False
            curves[j0:j0 + m, it] = np.stack([S.sum(1), I.sum(1), R.sum(1)], axis=1)
    return t_inf, t_rec, curves


def counts_from_events(t_inf, t_rec, T):
    """uint32 [3, T, n]: the events histogrammed into what `sir_philox` accumulates, row-0 quirk included."""
    t = np.arange(T)[:, None, None]
    inf = (t_inf[None] >= 0) & (t_inf[None] <= t)
    rec = (t_rec[None] >= 0) & (t_rec[None] <= t)
    cnt = np.stack([(~inf).sum(1), (inf & ~rec).sum(1), rec.sum(1)]).astype(np.uint32)
    seeded = (t_inf == 0).any(0)
    cnt[0, 0], cnt[1, 0], cnt[2, 0] = ~seeded, seeded, 0
    return cnt


def states_at(t_inf, t_rec, t):
    """int8 [sims, n]: 0 S, 1 I, 2 R at step t."""
    return (((t_inf >= 0) & (t_inf <= t)).astype(np.int8) + ((t_rec >= 0) & (t_rec <= t)).astype(np.int8))
