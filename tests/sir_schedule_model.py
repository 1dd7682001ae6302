"""The CPU model of the Monte-Carlo SIR with rates that change over time (a helper, not a test): `sir_model.sir_events` with the
infection and recovery thresholds chosen per step.

A call over T grid points takes steps t = 1 .. T-1; phase[t] in [0, P) names the tables that govern step t (entry 0 is never
read).  In step t, on the pre-step state, the entry at CSR position q (row u infected, col[q] = v susceptible) fires iff
coin(q, t, sim, kind 0) < THR[phase[t]][q], and the infected u recovers iff coin(u, t, sim, kind 1) < TG[phase[t]][u].  Coins,
thresholds and the drawn start are sir_model's; tests/test_schedule_model.py holds a schedule of one phase to `sir_events`."""
import numpy as np

import sir_model as M
from gnode_oracle import philox_coin


def schedule_thresholds(W, G, nnz, n):
    """(THR, TG): per phase, uint64 [nnz] of the per-position weights W[p] and uint64 [n] of the recovery rates G[p] (a number
    or per node)."""
    return [M.thresholds(w, nnz) for w in W], [M.thresholds(g, n) for g in G]


def sir_events_schedule(n, rowptr, col, start, THR, TG, phase, sims, T, rng_seed, sim_offset=0):
    """(t_inf, t_rec), int16 [sims, n], as `sir_model.sir_events` returns them; `start` is a seed list or p [n, 3]."""
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    dst = np.asarray(col).astype(np.int64)
    nnz = dst.shape[0]
    eid = np.arange(nnz, dtype=np.uint64)
    k0, k1 = np.uint64(rng_seed & 0xFFFFFFFF), np.uint64((rng_seed >> 32) & 0xFFFFFFFF)
    drawn = np.ndim(start) == 2
    if drawn:
        tS, tR = M.init_thresholds(start)
    t_inf = np.full((sims, n), -1, dtype=np.int16)
    t_rec = np.full((sims, n), -1, dtype=np.int16)
    chunk = max(1, min(sims, 4_000_000 // max(nnz, n, 1)))
    for c0 in range(0, sims, chunk):
        ss = np.arange(sim_offset + c0, sim_offset + min(c0 + chunk, sims), dtype=np.uint64)
        ti, tr = t_inf[c0:c0 + len(ss)], t_rec[c0:c0 + len(ss)]
        if drawn:
            st = M.draw_initial_state(tS, tR, ss, k0, k1)
        else:
            st = np.zeros((len(ss), n), dtype=np.int8)
            st[:, list(start)] = 1
        S, I, R = st == 0, st == 1, st == 2
        ti[~S] = 0
        tr[R] = 0
        for it in range(1, T):
            thr, tg = THR[phase[it]], TG[phase[it]]                # this step's tables
            ak, ae = np.nonzero(I[:, src] & S[:, dst])             # (trajectory, CSR entry), decided on the pre-step state
            fire = philox_coin(eid[ae], it, ss[ak], 0, k0, k1) < thr[ae]
            ik, iu = np.nonzero(I)
            gone = philox_coin(iu.astype(np.uint64), it, ss[ik], 1, k0, k1) < tg[iu]
            nk, nv, rk, ru = ak[fire], dst[ae[fire]], ik[gone], iu[gone]
            R[rk, ru] = True
            I[nk, nv] = True; I[rk, ru] = False; S[nk, nv] = False
            ti[nk, nv] = it
            tr[rk, ru] = it
    return t_inf, t_rec
