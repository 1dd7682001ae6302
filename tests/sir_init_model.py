"""CPU references of the baselines started from an initial-state distribution (a helper, not a test): DMP and the mean-field
from p, float64 [n, 3] = (pS, pI, pR) per node, the per-cell bound that holds Monte-Carlo counts to marginals, and the tree
case's start.  The Monte-Carlo model itself is tests/sir_model.py; tests/test_sir_init_model.py holds `dmp_sir_init` to `dmp_sir`."""
import numpy as np

from gnode_oracle import dmp_reverse_index
from sir_model import mixed_init


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
