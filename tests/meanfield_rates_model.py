"""CPU model of the mean-field with per-node and per-contact rates (a helper, not a test): one sample per call.

    dS_v = -beta[v] S_v sum_u M[u, v] I_u,   dI_v = -dS_v - gamma[v] I_v,   dR_v = gamma[v] I_v

M[u, v] = w[p] for the CSR position p of row u with col[p] = v: the rate at which u infects v (source = row, target =
column, the convention of `gnode.ode_nn.edge_rates` and `DMP_SIR`).  The in-weights of node v are therefore column v of M:
the model multiplies I by the TRANSPOSE of the weight matrix.  scipy's odeint at rtol = atol = 1e-11, the yardstick of the
project's 1e-6 mean-field bar (tests/test_gpu_baselines.py, `sir_init_model.meanfield_init`);
tests/test_meanfield_rates_model.py holds it to the reference's own `runge_kutta_order4` on the dense transpose."""
import numpy as np

MF_ATOL = 1e-6                  # the project's mean-field bar, absolute on probabilities


def in_weight_matrix(rowptr, col, w=None):
    """scipy CSR [n, n] whose row v holds the in-weights of v: (M^T)[v, u] = M[u, v]; w None = every stored entry 1."""
    import scipy.sparse as sp
    n = len(rowptr) - 1
    w = np.ones(len(col)) if w is None else np.asarray(w, dtype=np.float64)
    return sp.csr_matrix((w, np.asarray(col), np.asarray(rowptr)), shape=(n, n)).T.tocsr()


def sample_times(deltaT, maxTime):
    """The reference's sampling (ode_nn.py:227-232, 243-245): row i of the result is the solution at grid[int(i / deltaT)]."""
    grid = np.arange(0, maxTime, deltaT)
    return grid, [int(i / deltaT) for i in range(int(maxTime))]


def meanfield_rates(rowptr, col, p, beta, w, gamma, maxTime, deltaT=1):
    """(I, S, R), float64 [maxTime, n], from y(0) = p ([n, 3] = (pS, pI, pR)).  beta: a number, [n] (indexed by the target
    node) or None = 1; w: [nnz] in CSR position order or None = 1; gamma: a number or [n]."""
    from scipy.integrate import odeint
    n = len(rowptr) - 1
    At = in_weight_matrix(rowptr, col, w)
    bet = np.ones(n) if beta is None else np.asarray(beta, dtype=np.float64) * np.ones(n)
    gam = np.asarray(gamma, dtype=np.float64) * np.ones(n)

    def rhs(x, t):
        S, I = x[:n], x[n:2 * n]
        dS = -bet * (At @ I) * S
        return np.hstack([dS, -dS - gam * I, gam * I])

    p = np.asarray(p, dtype=np.float64)
    grid, rows = sample_times(deltaT, maxTime)
    sol = odeint(rhs, np.hstack([p[:, 0], p[:, 1], p[:, 2]]), grid, rtol=1e-11, atol=1e-11)[rows]
    return sol[:, n:2 * n], sol[:, :n], sol[:, 2 * n:]


def one_hot(n, seeds):
    p = np.zeros((n, 3))
    p[:, 0] = 1.0
    p[list(seeds)] = (0.0, 1.0, 0.0)
    return p


def golden_case(name):
    """A golden file of tests/golden/make_golden_meanfield_rates.py as a dict; beta / w are None where the case has none."""
    import os
    d = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"meanfield_rates_{name}.npz")))
    d["beta"] = d["beta"] if d["beta"].size else None
    d["w"] = d["w"] if d["w"].size else None
    d["seeds"] = [int(s) for s in d["seeds"]]
    d["deltaT"] = float(d["deltaT"]) if float(d["deltaT"]) != int(d["deltaT"]) else int(d["deltaT"])
    d["maxTime"] = int(d["maxTime"])
    return d


def max_diff(got, want):
    return max(float(np.max(np.abs(np.asarray(g) - np.asarray(w)))) for g, w in zip(got, want))
