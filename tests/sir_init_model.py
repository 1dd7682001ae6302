"""CPU models of the label generator and the baselines started from an initial-state distribution (a helper, not a test).

`p` is float64 [n, 3] = (pS, pI, pR) per node.  Monte-Carlo: each trajectory draws its own start, independently per node --
with coin = philox_coin(v, step 0, sim, kind 2), tS = thr(pS), tR = thr(pR), thr(p) = floor(p * 2^32), node v starts in S
iff coin < tS, else in R iff coin >= 2^32 - tR, else in I (64-bit compares) -- and steps 1 .. T-1 are the loop of
tests/sir_edges_model.py, run for a batch of trajectories at a time.  Row 0 of the counts is accumulated like every other
row.  Coins and thresholds are the oracle's; tests/test_sir_init_model.py holds this helper to `sir_philox`,
`sir_philox_edges` and `dmp_sir`."""
import numpy as np

from gnode_oracle import coin_threshold, dmp_reverse_index, philox_coin
from sir_nodes_model import thresholds

TWO32 = np.uint64(1 << 32)


def init_thresholds(p):
    """(tS, tR): uint64 [n] each."""
    p = np.asarray(p, dtype=np.float64)
    return (np.asarray([coin_threshold(x) for x in p[:, 0]], dtype=np.uint64),
            np.asarray([coin_threshold(x) for x in p[:, 2]], dtype=np.uint64))


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


def sir_philox_init(n, rowptr, col, p, w, gamma, sims, T, rng_seed, sim_offset=0, return_events=False):
    """uint32 counts [3, T, n] (S, I, R), row 0 accumulated, for w[p] per CSR position (a constant is the scalar form,
    beta[col] the per-node form) and gamma per node (a scalar broadcasts); with return_events also int16 t_inf, t_rec
    [sims, n]: a node that starts in I has t_inf = 0, one that starts in R has t_inf = t_rec = 0."""
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    dst = np.asarray(col).astype(np.int64)
    nnz = dst.shape[0]
    eid = np.arange(nnz, dtype=np.uint64)
    k0, k1 = np.uint64(rng_seed & 0xFFFFFFFF), np.uint64((rng_seed >> 32) & 0xFFFFFFFF)
    tw = np.asarray([coin_threshold(x) for x in np.broadcast_to(np.asarray(w, dtype=np.float64), (nnz,))], dtype=np.uint64)
    tg = thresholds(gamma, n)
    tS, tR = init_thresholds(p)
    cnt = np.zeros((3, T, n), dtype=np.uint32)
    t_inf = np.full((sims, n), -1, dtype=np.int16)
    t_rec = np.full((sims, n), -1, dtype=np.int16)
    chunk = max(1, min(sims, 4_000_000 // max(nnz, n, 1)))         # trajectories stepped together (the coins do not care)
    for c0 in range(0, sims, chunk):
        ss = np.arange(sim_offset + c0, sim_offset + min(c0 + chunk, sims), dtype=np.uint64)
        ti, tr = t_inf[c0:c0 + len(ss)], t_rec[c0:c0 + len(ss)]
        st = draw_initial_state(tS, tR, ss, k0, k1)
        S, I, R = st == 0, st == 1, st == 2
        ti[~S] = 0
        tr[R] = 0
        cnt[0, 0] += S.sum(0, dtype=np.uint32); cnt[1, 0] += I.sum(0, dtype=np.uint32); cnt[2, 0] += R.sum(0, dtype=np.uint32)
        for it in range(1, T):
            ak, ae = np.nonzero(I[:, src] & S[:, dst])             # decided on the pre-step state
            fire = philox_coin(eid[ae], it, ss[ak], 0, k0, k1) < tw[ae]
            ik, iu = np.nonzero(I)
            gone = philox_coin(iu.astype(np.uint64), it, ss[ik], 1, k0, k1) < tg[iu]
            nk, nv, rk, ru = ak[fire], dst[ae[fire]], ik[gone], iu[gone]
            R[rk, ru] = True
            I[nk, nv] = True; I[rk, ru] = False; S[nk, nv] = False
            ti[nk, nv] = it
            tr[rk, ru] = it
            cnt[0, it] += S.sum(0, dtype=np.uint32); cnt[1, it] += I.sum(0, dtype=np.uint32); cnt[2, it] += R.sum(0, dtype=np.uint32)
    return (cnt, t_inf, t_rec) if return_events else cnt


def dmp_sir_init(rowptr, col, weights, gamma, p, maxTime, dtype="float32"):
    """`gnode_oracle.dmp_sir` from Ps_0 = pS, Pi_0 = pI, Pr_0 = pR with Phi_ij_0 = Pi_0[src] and Pr_1 = Pr_0 + gamma Pi_0;
    everything after that, the operation order and the 1e-10 offset included, as there.  float32 is the restatement the
    kernel is held to, float64 the yardstick."""
    f = np.dtype(dtype).type
    n, E = len(rowptr) - 1, len(col)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    tar = np.asarray(col, dtype=np.int64)
    cave = dmp_reverse_index(rowptr, col)
    w = np.asarray(weights, dtype=f)
    g_node = np.asarray(gamma, dtype=f)
    g_edge = g_node[src]

    def scatter_mul(vals, index, size):
        out = np.ones(size, dtype=f)
        np.multiply.at(out, index, np.asarray(vals, dtype=f))
        return out

    def mulmul(theta):
        P = scatter_mul(theta, tar, n)[src]
        cav = scatter_mul(theta, cave, E + 1)[:E]
        return (P / cav).astype(f)

    p = np.asarray(p, dtype=f)
    Ps0, Pi0, Pr0 = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    Ps_i0 = Ps0[src]
    Phi = Pi0[src]
    theta = ((np.ones(E, dtype=f) - w * Phi).astype(f) + f(1e-10)).astype(f)
    Ps_prev = Ps_i0
    Ps_e = (Ps_i0 * mulmul(theta)).astype(f)
    Phi = ((f(1) - w) * (f(1) - g_edge) * Phi - (Ps_e - Ps_prev)).astype(f)
    Ps_t = (Ps0 * scatter_mul(theta, tar, n)).astype(f)
    Pr_t = (Pr0 + g_node * Pi0).astype(f)
    Pi_t = (f(1) - Ps_t - Pr_t).astype(f)
    out = [np.stack([Ps0, Pi0, Pr0], 1), np.stack([Ps_t, Pi_t, Pr_t], 1)]
    for _ in range(maxTime - 2):
        theta = (theta - w * Phi).astype(f)
        new_Ps = (Ps_i0 * mulmul(theta)).astype(f)
        Ps_prev, Ps_e = Ps_e, new_Ps
        Phi = ((f(1) - w) * (f(1) - g_edge) * Phi - (Ps_e - Ps_prev)).astype(f)
        Ps_t = (Ps0 * scatter_mul(theta, tar, n)).astype(f)
        Pr_t = (Pr_t + g_node * Pi_t).astype(f)
        Pi_t = (f(1) - Ps_t - Pr_t).astype(f)
        out.append(np.stack([Ps_t, Pi_t, Pr_t], 1))
    return np.stack(out, 0).astype(f)


def meanfield_init(rowptr, col, p, beta, gamma, maxTime):
    """The mean-field reference from y(0) = (pS, pI, pR): scipy's odeint at rtol = atol = 1e-11 on t = 0 .. maxTime - 1, as
    `gnode_oracle.meanfield_rk` is called by the baseline tests.  Returns (I, S, R), float64 [maxTime, n]."""
    import scipy.sparse as sp
    from scipy.integrate import odeint
    n = len(rowptr) - 1
    A = sp.csr_matrix((np.ones(len(col)), np.asarray(col), np.asarray(rowptr)), shape=(n, n))
    gam = np.asarray(gamma, dtype=np.float64) * np.ones(n)

    def rhs(x, t):
        S, I = x[:n], x[n:2 * n]
        dS = -beta * (A @ I) * S
        return np.hstack([dS, -dS - gam * I, gam * I])

    p = np.asarray(p, dtype=np.float64)
    sol = odeint(rhs, np.hstack([p[:, 0], p[:, 1], p[:, 2]]), np.arange(0, maxTime, 1), rtol=1e-11, atol=1e-11)
    return sol[:, n:2 * n], sol[:, :n], sol[:, 2 * n:]


def sigma_ratio(counts, sims, P, rows=slice(None)):
    """max over the cells of the given rows of |count / sims - P| / (sqrt(P (1 - P) / sims) + 1 / sims); counts uint32
    [3, T, n], P float64 [T, n, 3].  The project's bound is a ratio of at most 5."""
    f = counts[:, rows].astype(np.float64).transpose(1, 2, 0) / sims
    p = np.clip(P[rows], 0.0, 1.0)
    return float(np.max(np.abs(f - P[rows]) / (np.sqrt(p * (1.0 - p) / sims) + 1.0 / sims)))


def tree_init():
    """The initial state of the tree case: `mixed_init(120, 11)`, 74 / 4 / 12 / 30 nodes of the four kinds."""
    p, kind = mixed_init(120, 11)
    assert np.bincount(kind, minlength=4).tolist() == [74, 4, 12, 30]
    return p
