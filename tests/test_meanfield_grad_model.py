"""CPU: the numpy model of the differentiable mean-field (tests/meanfield_grad_model.py) is held to three yardsticks before the
GPU tests lean on it: its adaptive forward to the project's odeint model, its reverse rule to central differences of its own
replay, and the frozen-step gradient to the continuous ODE's forward sensitivities.  The float64 rounding bar of the GPU tests,
MF_GRAD_RTOL, is measured here against np.longdouble."""
import numpy as np
import pytest

import meanfield_grad_model as M
from meanfield_rates_model import MF_ATOL, meanfield_rates

from meanfield_grad_model import MEASURED_F64_ROUNDING, MF_GRAD_RTOL

# The frozen-step gradient against the true one (karate, odeint sensitivities at 1e-11): measured gap 3.95e-11, bar 10 x
MEASURED_SENS_GAP = 3.95e-11
SENS_BAR = 10 * MEASURED_SENS_GAP

FD_EPS, FD_BAR = 1e-6, 1e-6             # central differences: eps^2 truncation plus 1e-16 / eps rounding are the limiting side


def _karate():
    import networkx as nx
    e = np.array(nx.karate_club_graph().edges())
    return M._sym_csr(34, e[:, 0], e[:, 1])


def test_adaptive_forward_meets_the_odeint_model():
    rp, ci = M.random_graph(40, 100, 1)
    case = M._inputs(rp, ci, 2, 2)
    t_out = M._times(1, 8)
    (I, S, R), h, n_acc, steps = M.dp5_adaptive(rp, ci, case["init"], case["beta"], case["gamma"], case["w"], t_out)
    assert n_acc[0] == 0 and n_acc.sum() == len(h) <= steps and (n_acc[1:] > 0).all()
    for b in range(2):
        want = meanfield_rates(rp, ci, case["init"][b], case["beta"][b], case["w"], case["gamma"][b], 8)
        for got, w in zip((I, S, R), want):
            assert np.max(np.abs(got[:, b] - w)) <= MF_ATOL
    again = M.dp5_replay(rp, ci, case["init"], case["beta"], case["gamma"], case["w"], len(t_out), h, n_acc)
    for a, b in zip(again, (I, S, R)):
        assert np.array_equal(a, b)                                 # the replay walks the same arithmetic


def _loss(case, n_out, h, n_acc, g, **over):
    a = {**case, **over}
    I, S, R = M.dp5_replay(a["rp"], a["ci"], a["init"], a["beta"], a["gamma"], a["w"], n_out, h, n_acc)
    return float((g[0] * I).sum() + (g[1] * S).sum() + (g[2] * R).sum())


@pytest.mark.parametrize("loops,zero_w", [((), False), ((1,), True)], ids=["plain", "loop_directed"])
def test_reverse_rule_meets_central_differences(loops, zero_w):
    """every entry of every gradient, steps frozen; a repeated output time and a self-loop among the cases"""
    rp, ci = M.random_graph(6, 9, 3, loops=loops)
    case = M._inputs(rp, ci, 2, 4, zero_w=zero_w)
    t_out = np.array([0.0, 1.0, 1.0, 2.5])
    _, h, n_acc, _ = M.dp5_adaptive(rp, ci, case["init"], case["beta"], case["gamma"], case["w"], t_out, rtol=1e-6, atol=1e-8)
    g = M.grad_out(dict(case, t_out=t_out))
    got = M.dp5_replay_grad(rp, ci, case["init"], case["beta"], case["gamma"], case["w"], len(t_out), h, n_acc, *g)
    for key in ("init", "beta", "gamma", "w"):
        base = case[key]
        fd = np.zeros(base.shape)
        for idx in np.ndindex(*base.shape):
            lo, hi = base.copy(), base.copy()
            lo[idx] -= FD_EPS
            hi[idx] += FD_EPS
            fd[idx] = (_loss(case, len(t_out), h, n_acc, g, **{key: hi}) - _loss(case, len(t_out), h, n_acc, g, **{key: lo})) / (2 * FD_EPS)
        mine = got[key].sum(0) if key == "w" else got[key]          # w is shared: its gradient is the sum of the samples' rows
        assert np.max(np.abs(fd)) > 0
        assert M.rel_err(mine, fd) <= FD_BAR, key
    for b in range(2):                                              # a sample's row of grad_w is its solo run's
        one = {k: (v if v is None or k in ("rp", "ci", "w") else v[b:b + 1]) for k, v in case.items()}
        solo = M.dp5_replay_grad(rp, ci, one["init"], one["beta"], one["gamma"], one["w"], len(t_out), h, n_acc, *(x[:, b:b + 1] for x in g))
        assert np.array_equal(solo["w"][0], got["w"][b])


def _sensitivity_grads(rp, ci, case, t_out, g):
    """the gradient of the linear loss through scipy's odeint on the continuous ODE and its forward sensitivities, one sample"""
    from scipy.integrate import odeint
    n, nnz = len(rp) - 1, len(ci)
    src, _ = M.tables(rp, ci)
    Wt = np.zeros((n, n))
    Wt[ci, src] = case["w"]                                         # Wt[v, u]: the rate at which u infects v
    bet, gam, p = case["beta"][0], case["gamma"][0], case["init"][0]
    y0 = np.hstack([p[:, 0], p[:, 1], p[:, 2]])
    names = [("init", (v, c)) for v in range(n) for c in range(3)] + [("beta", v) for v in range(n)] + [("gamma", v) for v in range(n)] + [("w", q) for q in range(nnz)]
    out = {"init": np.zeros((n, 3)), "beta": np.zeros(n), "gamma": np.zeros(n), "w": np.zeros(nnz)}
    for lo in range(0, len(names), 48):
        chunk = names[lo:lo + 48]
        m = len(chunk)
        s0 = np.zeros((3 * n, m))
        for k, (kind, i) in enumerate(chunk):
            if kind == "init":
                s0[[0, n, 2 * n][i[1]] + i[0], k] = 1.0

        def rhs(x, t):
            y, s = x[:3 * n], x[3 * n:].reshape(3 * n, m)
            S, I = y[:n], y[n:2 * n]
            ai = Wt @ I
            inf, rec = bet * ai * S, gam * I
            dinf = bet[:, None] * (ai[:, None] * s[:n] + S[:, None] * (Wt @ s[n:2 * n]))
            drec = gam[:, None] * s[n:2 * n]
            for k, (kind, i) in enumerate(chunk):
                if kind == "beta":
                    dinf[i, k] += ai[i] * S[i]
                elif kind == "gamma":
                    drec[i, k] += I[i]
                elif kind == "w":
                    dinf[ci[i], k] += bet[ci[i]] * S[ci[i]] * I[src[i]]
            return np.hstack([-inf, inf - rec, rec, np.vstack([-dinf, dinf - drec, drec]).reshape(-1)])

        sol = odeint(rhs, np.hstack([y0, s0.reshape(-1)]), np.unique(t_out), rtol=1e-11, atol=1e-11)
        rows = np.searchsorted(np.unique(t_out), t_out)
        s = sol[rows, 3 * n:].reshape(len(t_out), 3, n, m)           # planes S, I, R
        val = np.einsum("tv,tvk->k", g[1][:, 0], s[:, 0]) + np.einsum("tv,tvk->k", g[0][:, 0], s[:, 1]) + np.einsum("tv,tvk->k", g[2][:, 0], s[:, 2])
        for k, (kind, i) in enumerate(chunk):
            out[kind][i] = val[k]
    return out


def _sens_gap():
    rp, ci = _karate()
    case = M._inputs(rp, ci, 1, 21)
    t_out = M._times(1, 5)
    _, h, n_acc, _ = M.dp5_adaptive(rp, ci, case["init"], case["beta"], case["gamma"], case["w"], t_out)
    g = M.grad_out(dict(case, t_out=t_out))
    got = M.dp5_replay_grad(rp, ci, case["init"], case["beta"], case["gamma"], case["w"], len(t_out), h, n_acc, *g)
    want = _sensitivity_grads(rp, ci, case, t_out, g)
    return max(M.rel_err(got[k][0], want[k]) for k in ("init", "beta", "gamma", "w"))


def test_frozen_step_gradient_is_the_true_gradient():
    gap = _sens_gap()
    print(f"frozen-step gradient against odeint sensitivities, karate: {gap:.3e} (bar {SENS_BAR:.3e})")
    assert gap <= SENS_BAR


def f64_rounding():
    """the largest float64-against-longdouble distance over the GPU cases: outputs and every gradient array"""
    worst = 0.0
    for name, c in M.gpu_cases().items():
        n_out = len(c["t_out"])
        _, h, n_acc, _ = M.dp5_adaptive(c["rp"], c["ci"], c["init"], c["beta"], c["gamma"], c["w"], c["t_out"], M.RTOL, M.ATOL)
        g = M.grad_out(c)
        args = (c["rp"], c["ci"], c["init"], c["beta"], c["gamma"], c["w"], n_out, h, n_acc)
        lo, hi = M.dp5_replay_grad(*args, *g), M.dp5_replay_grad(*args, *g, dtype=np.longdouble)
        for key in M.compared_keys(c):
            want = hi[key]
            if n_out > 1 or key == "init":
                assert np.max(np.abs(want)) > 0, (name, key)        # a case only counts where the model's gradient is not 0
            if np.max(np.abs(want)) > 0:
                worst = max(worst, M.rel_err(lo[key], want))
        for a, b in zip(M.dp5_replay(*args), M.dp5_replay(*args, dtype=np.longdouble)):
            worst = max(worst, M.rel_err(a, b))
    return worst


def test_float64_rounding_bar():
    assert np.finfo(np.longdouble).eps < 1e-18                      # the yardstick is wider than float64 here
    worst = f64_rounding()
    print(f"float64 against longdouble over the GPU cases: {worst:.3e}; MF_GRAD_RTOL = {MF_GRAD_RTOL:.3e}")
    assert 0 < worst <= MEASURED_F64_ROUNDING
    assert MF_GRAD_RTOL == 64 * MEASURED_F64_ROUNDING
