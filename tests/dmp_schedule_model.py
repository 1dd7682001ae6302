"""The CPU reference of DMP with rates that change over time (a helper, not a test): `sir_init_model.dmp_sir_init` with the
weights and recovery probabilities chosen per step, float32 (the restatement the kernels are held to) and float64 (the
yardstick).

Step t = 1 .. maxTime-1 leads from state t-1 to state t under tables W[phase[t]] [nnz], G[phase[t]] [n]:
  theta_1     = (1 - w^{phase[1]} phi_0) + 1e-10
  step t        Ps_e(t) = Ps0[src] * cavity product of theta_t
                phi_t = (1 - w^{phase[t]})(1 - gamma^{phase[t]}_src) phi_{t-1} - (Ps_e(t) - Ps_e(t-1))
                Ps_t = Ps0 * product of theta_t;  Pr_t = Pr_{t-1} + gamma^{phase[t]} Pi_{t-1};  Pi_t = 1 - Ps_t - Pr_t
                theta_{t+1} = theta_t - w^{phase[t+1]} phi_t          (when t + 1 < maxTime)
phi_t, what survived step t, reads step t's tables; theta_{t+1} - theta_t, what is transmitted during step t + 1, reads that
step's weight.  variant="this" takes theta_{t+1}'s weight from step t instead: the wrong recurrence, kept so that the tests
can show that the Monte-Carlo tells the two apart."""
import numpy as np

from gnode_oracle import dmp_reverse_index


def dmp_sir_schedule(rowptr, col, W, G, phase, p, maxTime, dtype="float32", variant="next"):
    f = np.dtype(dtype).type
    n, E = len(rowptr) - 1, len(col)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    tar = np.asarray(col, dtype=np.int64)
    cave = dmp_reverse_index(rowptr, col)

    def scatter_mul(vals, index, size):
        out = np.ones(size, dtype=f)
        np.multiply.at(out, index, np.asarray(vals, dtype=f))
        return out

    def mulmul(theta):
        P = scatter_mul(theta, tar, n)[src]
        cav = scatter_mul(theta, cave, E + 1)[:E]
        return (P / cav).astype(f)

    def tables(t):
        return np.asarray(W[phase[t]], dtype=f) * np.ones(E, dtype=f), np.asarray(G[phase[t]], dtype=f) * np.ones(n, dtype=f)

    p = np.asarray(p, dtype=f)
    Ps0, Pi_t, Pr_t = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    Ps_i0 = Ps0[src]
    Phi = Pi_t[src]
    Ps_e = Ps_i0
    out = [np.stack([Ps0, Pi_t, Pr_t], 1)]
    theta = ((np.ones(E, dtype=f) - tables(1)[0] * Phi).astype(f) + f(1e-10)).astype(f)
    for t in range(1, maxTime):
        w, g_node = tables(t)
        new_Ps = (Ps_i0 * mulmul(theta)).astype(f)
        Phi = ((f(1) - w) * (f(1) - g_node[src]) * Phi - (new_Ps - Ps_e)).astype(f)
        Ps_e = new_Ps
        Ps_t = (Ps0 * scatter_mul(theta, tar, n)).astype(f)
        Pr_t = (Pr_t + g_node * Pi_t).astype(f)
        Pi_t = (f(1) - Ps_t - Pr_t).astype(f)
        out.append(np.stack([Ps_t, Pi_t, Pr_t], 1))
        if t + 1 < maxTime:
            w_next = tables(t + 1)[0] if variant == "next" else w
            theta = (theta - w_next * Phi).astype(f)
    return np.stack(out, 0).astype(f)
