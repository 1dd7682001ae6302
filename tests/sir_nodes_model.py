"""CPU model of the Monte-Carlo SIR labels with per-node rates (a helper, not a test).

The loop of `oracle.gnode_oracle.sir_philox` with two numbers turned into arrays: the infection coin of the directed CSR
entry (u -> v) is held against the threshold of its TARGET v, the recovery coin of node u against u's own.  Coins and
thresholds are the oracle's (`philox_coin`, `coin_threshold`); tests/test_sir_nodes_model.py holds this helper to
`sir_philox` itself."""
import numpy as np

from gnode_oracle import coin_threshold, philox_coin


def thresholds(p, n):
    """uint64 [n] of `coin_threshold` values from one rate or n rates."""
    return np.asarray([coin_threshold(x) for x in np.broadcast_to(np.asarray(p, dtype=np.float64), (n,))], dtype=np.uint64)


def sir_philox_nodes(n, rowptr, col, seed_set, beta, gamma, sims, T, rng_seed, sim_offset=0):
    """uint32 counts [3, T, n] (S, I, R), row-0 quirk included, for beta[v] / gamma[u] per node (a scalar broadcasts)."""
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    dst = col.astype(np.int64)
    eid = np.arange(col.shape[0], dtype=np.uint64)
    k0, k1 = np.uint64(rng_seed & 0xFFFFFFFF), np.uint64((rng_seed >> 32) & 0xFFFFFFFF)
    tb, tg = thresholds(beta, n), thresholds(gamma, n)
    cnt = np.zeros((3, T, n), dtype=np.uint32)
    for s in range(sim_offset, sim_offset + sims):
        I = np.zeros(n, dtype=bool); S = np.ones(n, dtype=bool); R = np.zeros(n, dtype=bool)
        I[list(seed_set)] = True; S[list(seed_set)] = False
        cnt[0, 0] = S; cnt[1, 0] = I
        for it in range(1, T):
            act = np.nonzero(I[src] & S[dst])[0]
            w = philox_coin(eid[act], it, s, 0, k0, k1)
            new_inf = dst[act[w < tb[dst[act]]]]
            idx_I = np.nonzero(I)[0]
            w2 = philox_coin(idx_I.astype(np.uint64), it, s, 1, k0, k1)
            new_rec = idx_I[w2 < tg[idx_I]]
            R[new_rec] = True
            I[new_inf] = True; I[new_rec] = False; S[new_inf] = False
            cnt[0, it] += S; cnt[1, it] += I; cnt[2, it] += R
    return cnt
