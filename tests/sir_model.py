"""The CPU model of the Monte-Carlo SIR label generator (a helper, not a test): ONE step loop for every rate form, start and
output.

The loop of `gnode_oracle.sir_philox`, run for a block of trajectories at a time, with
  * the infection threshold taken at the CSR position: the directed entry at position q, in row u with col[q] = v, fires iff
    coin(q, step, sim, kind 0) < thr[q] (`infection_thresholds`: a scalar beta, a per-node beta looked up at the TARGET v, or
    the per-entry weights w[q], the probability that the row u infects the column v);
  * the recovery coin of node u, coin(u, step, sim, kind 1), held against u's own gamma;
  * the start either a seed list or a distribution p, float64 [n, 3] = (pS, pI, pR), drawn per trajectory and node with
    coin(v, step 0, sim, kind 2): S iff coin < thr(pS), else R iff coin >= 2^32 - thr(pR), else I (64-bit compares).
It returns the events.  Counts, curves and states are folded from them (`counts`, `curves`, `states_at`).  Coins and
thresholds are the oracle's (`philox_coin`, `coin_threshold`); tests/test_sir_model.py holds the model to `sir_philox`, to
`dmp_sir`, to closed forms and to the outputs of the four models it replaced (tests/golden/sir_model_parent.json)."""
import numpy as np

from gnode_oracle import coin_threshold, philox_coin

TWO32 = np.uint64(1 << 32)


def thresholds(p, size):
    """uint64 [size] of `coin_threshold` values from one probability or `size` of them."""
    return np.asarray([coin_threshold(x) for x in np.broadcast_to(np.asarray(p, dtype=np.float64), (size,))], dtype=np.uint64)


def infection_thresholds(n, col, beta=None, w=None):
    """uint64 [nnz], one per CSR position: of `beta`, a scalar or per node (the target's: thr(beta)[col]), or of `w`, per
    position."""
    assert (beta is None) != (w is None)
    if w is not None:
        return thresholds(w, len(col))
    return thresholds(beta, len(col)) if np.ndim(beta) == 0 else thresholds(beta, n)[np.asarray(col, dtype=np.int64)]


def init_thresholds(p):
    """(tS, tR): uint64 [n] each."""
    p = np.asarray(p, dtype=np.float64)
    return thresholds(p[:, 0], len(p)), thresholds(p[:, 2], len(p))


def draw_initial_state(tS, tR, sim, k0, k1):
    """int8, 0 S / 1 I / 2 R: [n] for one trajectory `sim`, [m, n] for an array of m of them."""
    n = tS.shape[0]
    sims = np.atleast_1d(np.asarray(sim, dtype=np.uint64))
    pos = np.broadcast_to(np.arange(n, dtype=np.uint64), (sims.shape[0], n))
    coin = philox_coin(pos.ravel(), 0, np.repeat(sims, n), 2, k0, k1).reshape(sims.shape[0], n)
    st = np.where(coin < tS, 0, np.where(coin >= TWO32 - tR, 2, 1)).astype(np.int8)
    return st if np.ndim(sim) else st[0]


def mixed_init(n, seed):
    """55 % one-hot S, 5 % one-hot I, 10 % one-hot R, 30 % Dirichlet(4, 1, 1) rows, in the draw order of the tree case."""
    rng = np.random.default_rng(seed)
    kind = rng.choice(4, size=n, p=[0.55, 0.05, 0.10, 0.30])
    p = np.zeros((n, 3))
    for k in range(3):
        p[kind == k, k] = 1.0
    d = rng.dirichlet([4, 1, 1], size=n)
    p[kind == 3] = d[kind == 3]
    return p, kind


def one_hot_init(n, infected, immune=()):
    p = np.zeros((n, 3))
    p[:, 0] = 1.0
    p[list(infected)] = (0.0, 1.0, 0.0)
    p[list(immune)] = (0.0, 0.0, 1.0)
    return p


def one_way_path(k):
    """(n, rowptr, col, w) of the line 0 - 1 - ... - k with w = 1 on every entry i -> i + 1 and 0 on every i + 1 -> i."""
    n = k + 1
    rows = [[j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.asarray([j for r in rows for j in r], dtype=np.int32)
    src = np.repeat(np.arange(n), np.diff(rowptr))
    return n, rowptr, col, (col > src).astype(np.float64)


def sir_events(n, rowptr, col, start, thr, gamma, sims, T, rng_seed, sim_offset=0):
    """(t_inf, t_rec), int16 [sims, n]: the step at which each node of the call's s-th trajectory (coins of sim_offset + s)
    left S and the step at which it recovered, -1 for never within T.  `start` is a seed list (a duplicate is one seed) or p
    [n, 3]: a node that starts in I has t_inf = 0, one that starts in R has t_inf = t_rec = 0.  `thr` is
    `infection_thresholds`; gamma is a scalar or per node."""
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    dst = np.asarray(col).astype(np.int64)
    nnz = dst.shape[0]
    eid = np.arange(nnz, dtype=np.uint64)
    k0, k1 = np.uint64(rng_seed & 0xFFFFFFFF), np.uint64((rng_seed >> 32) & 0xFFFFFFFF)
    tg = thresholds(gamma, n)
    drawn = np.ndim(start) == 2
    if drawn:
        tS, tR = init_thresholds(start)
    t_inf = np.full((sims, n), -1, dtype=np.int16)
    t_rec = np.full((sims, n), -1, dtype=np.int16)
    chunk = max(1, min(sims, 4_000_000 // max(nnz, n, 1)))         # trajectories stepped together (the coins do not care)
    for c0 in range(0, sims, chunk):
        ss = np.arange(sim_offset + c0, sim_offset + min(c0 + chunk, sims), dtype=np.uint64)
        ti, tr = t_inf[c0:c0 + len(ss)], t_rec[c0:c0 + len(ss)]
        if drawn:
            st = draw_initial_state(tS, tR, ss, k0, k1)
        else:
            st = np.zeros((len(ss), n), dtype=np.int8)
            st[:, list(start)] = 1
        S, I, R = st == 0, st == 1, st == 2
        ti[~S] = 0
        tr[R] = 0
        for it in range(1, T):
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


def _by_step(t_inf, t_rec, T):
    """(t, left S by t, recovered by t), bool [sims, n], step by step."""
    for t in range(T):
        yield t, (t_inf >= 0) & (t_inf <= t), (t_rec >= 0) & (t_rec <= t)


def counts(t_inf, t_rec, T, hold_row0):
    """uint32 [3, T, n] (S, I, R) over the trajectories.  hold_row0 is the seed-list calls' rule, `sir_philox`'s row-0 quirk:
    S and I row 0 hold the start ONCE and R row 0 is 0; without it (the calls that draw the start) row 0 is accumulated like
    every other row."""
    cnt = np.zeros((3, T, t_inf.shape[1]), dtype=np.uint32)
    for t, inf, rec in _by_step(t_inf, t_rec, T):
        cnt[0, t], cnt[1, t], cnt[2, t] = (~inf).sum(0), (inf & ~rec).sum(0), rec.sum(0)
    if hold_row0:
        seeded = (t_inf == 0).any(0)
        cnt[0, 0], cnt[1, 0], cnt[2, 0] = ~seeded, seeded, 0
    return cnt


def curves(t_inf, t_rec, T):
    """uint32 [sims, T, 3]: the population totals (S_t, I_t, R_t) of each trajectory, row 0 the true initial state."""
    cv = np.zeros((t_inf.shape[0], T, 3), dtype=np.uint32)
    for t, inf, rec in _by_step(t_inf, t_rec, T):
        cv[:, t, 0], cv[:, t, 1], cv[:, t, 2] = (~inf).sum(1), (inf & ~rec).sum(1), rec.sum(1)
    return cv


def states_at(t_inf, t_rec, t):
    """int8 [sims, n]: 0 S, 1 I, 2 R at step t."""
    return (((t_inf >= 0) & (t_inf <= t)).astype(np.int8) + ((t_rec >= 0) & (t_rec <= t)).astype(np.int8))
