"""float64 torch restatements of the RHS vector-Jacobian product and of the RK4 (3/8 rule) adjoint, and the inputs of
the fixtures tests/golden/make_golden_rhs_vjp.py / make_golden_rk4_adjoint.py wrote (rebuilt from their seeds).

The VJP is written out from its formulas, not taken by autograd: the fixtures are autograd through the
reference's own ODEfunc, so agreement checks the formulas the kernel implements.  The RK4 adjoint restates torchdiffeq
0.2.2's odeint_adjoint(..., method='rk4') -- parity-unpinned, like the Euler rule of SURVEY Appendix A."""
from __future__ import annotations

import numpy as np
import torch


# --------------------------------------------------------------------------- fixture inputs
def vjp_inputs(rows: int, H: int, seed: int, sample_rows: int):
    """State y [4*rows, H] (S, I, R uniform in [0, 1.5); beta, gamma per sample in columns 0, 1 of the 4th slab, the other
    columns 0) and cotangent v (standard normal), float32.  sample_rows: rows per sample (beta, gamma are per sample)."""
    rng = np.random.default_rng(seed)
    y = rng.uniform(0, 1.5, size=(4 * rows, H)).astype(np.float32)
    y[3 * rows:] = 0.0
    B = rows // sample_rows
    y[3 * rows:, 0] = np.repeat(rng.uniform(0.1, 0.5, B), sample_rows)
    y[3 * rows:, 1] = np.repeat(rng.uniform(0.1, 0.5, B), sample_rows)
    v = rng.normal(size=(4 * rows, H)).astype(np.float32)
    return y, v


def multi_inputs(ns, picks, H: int, seed: int):
    """Multi-graph state [4, sumN, H] with the sample markers (graph index + 1 at each sample's first node, column 2 of the
    4th slab, ode_nn_ngraphs.py:55), and the cotangent."""
    rng = np.random.default_rng(seed)
    tot = sum(ns[p] for p in picks)
    y = rng.uniform(0, 1.5, size=(4, tot, H)).astype(np.float32)
    y[3] = 0.0
    o = 0
    for p in picks:
        y[3, o:o + ns[p], 0] = rng.uniform(0.1, 0.5)
        y[3, o:o + ns[p], 1] = rng.uniform(0.1, 0.5)
        y[3, o, 2] = p + 1
        o += ns[p]
    v = rng.normal(size=(4, tot, H)).astype(np.float32)
    return y, v


# --------------------------------------------------------------------------- RHS and its VJP
def _index(rowptr, col, n, rows):
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    B = rows // n
    ridx = torch.from_numpy(np.concatenate([src + b * n for b in range(B)]))
    cidx = torch.from_numpy(np.concatenate([col.astype(np.int64) + b * n for b in range(B)]))
    return ridx, cidx


def _spmm(ridx, cidx, T):
    return torch.zeros_like(T).index_add(0, ridx, T[cidx])


def rhs(y, W, b, ridx, cidx):
    """ODEfunc.forward (ode_nn_ngraph_sim.py:58-96) on torch tensors."""
    q = y.shape[0] // 4
    Z = torch.sigmoid(torch.nn.functional.linear(y[:2 * q], W, b))
    ZS, ZI = Z[:q], Z[q:]
    beta, gamma = y[3 * q:, 0:1], y[3 * q:, 1:2]
    AI = _spmm(ridx, cidx, ZI)
    dS = -beta * (AI * ZS)
    dI = -dS - gamma * ZI
    dR = gamma * ZI
    return torch.cat((dS, dI, dR, torch.zeros_like(y[3 * q:])))


def rhs_vjp(y, W, b, v, ridx, cidx):
    """(f, v^T df/dy, v^T df/dW, v^T df/db) from the formulas (A symmetric)."""
    q = y.shape[0] // 4
    yS, yI = y[:q], y[q:2 * q]
    Z = torch.sigmoid(torch.nn.functional.linear(y[:2 * q], W, b))
    ZS, ZI = Z[:q], Z[q:]
    beta, gamma = y[3 * q:, 0:1], y[3 * q:, 1:2]
    vS, vI, vR = v[:q], v[q:2 * q], v[2 * q:3 * q]
    AI = _spmm(ridx, cidx, ZI)
    u = beta * (vI - vS)
    dZS = u * AI
    dZI = _spmm(ridx, cidx, u * ZS) + gamma * (vR - vI)
    dS, dI = dZS * ZS * (1 - ZS), dZI * ZI * (1 - ZI)
    gy = torch.zeros_like(y)
    gy[:q], gy[q:2 * q] = dS @ W, dI @ W
    gy[3 * q:, 0] = ((vI - vS) * AI * ZS).sum(1)
    gy[3 * q:, 1] = ((vR - vI) * ZI).sum(1)
    gW = dS.T @ yS + dI.T @ yI
    gb = dS.sum(0) + dI.sum(0)
    f = torch.cat((-beta * (AI * ZS), beta * (AI * ZS) - gamma * ZI, gamma * ZI, torch.zeros_like(y[3 * q:])))
    return f, gy, gW, gb


def rhs_vjp_np(y, W, b, v, rowptr, col, n):
    """rhs_vjp in float64 on numpy inputs: (f, gy, gW, gb) as numpy."""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    ridx, cidx = _index(rowptr, col, n, y.shape[0] // 4)
    return tuple(o.numpy() for o in rhs_vjp(t(y), t(W), t(b), t(v), ridx, cidx))


# --------------------------------------------------------------------------- RK4 adjoint
def rk4_step(f, y, dt):
    """torchdiffeq 0.2.2 rk4_alt_step_func (3/8 rule): the increment of one step of size dt."""
    third = 1.0 / 3.0
    k1 = f(y)
    k2 = f(y + dt * k1 * third)
    k3 = f(y + dt * (k2 - k1 * third))
    k4 = f(y + dt * (k1 - k2 + k3))
    return (k1 + 3 * (k2 + k3) + k4) * dt * 0.125


def adjoint_grads(x, P, rowptr, col, maxTime, deltaT, loss_of_outputs, method="rk4", dtype=torch.float64):
    """The 8 parameter gradients of loss_of_outputs(S, I, R) (each [G, rows] torch) under torchdiffeq 0.2.2's
    odeint_adjoint: forward on the grid, then per interval i = G-1 .. 1 one step of size -dt of the augmented system
    (f, -a^T df/dy, -a^T df/dtheta) from t_i to t_{i-1}, y reset to sol[i-1], dL/dsol[i-1] added; a_0 into the encoder.
    method 'rk4' (3/8 rule) or 'euler'.  x [B, n, 3+H]."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    Pt = {k: t(v).requires_grad_(True) for k, v in P.items()}
    xt = t(x)
    n = xt.shape[1]
    x2 = xt.reshape(-1, xt.shape[2])
    rows = x2.shape[0]
    ridx, cidx = _index(rowptr, col, n, rows)
    W, b = Pt["odefunc.linear.weight"], Pt["odefunc.linear.bias"]
    enc = lambda s: torch.relu(torch.nn.functional.linear(s.unsqueeze(-1), Pt["linearS1.weight"], Pt["linearS1.bias"]))
    y0 = torch.cat((enc(x2[:, 0]), enc(x2[:, 1]), enc(x2[:, 2]), x2[:, 3:]))
    grid = np.arange(0, maxTime, deltaT)
    dts = (grid[1:] - grid[:-1]).astype(np.float32).astype(np.float64)
    f = lambda y: rhs(y, W.detach(), b.detach(), ridx, cidx)
    with torch.no_grad():
        sol = [y0.detach()]
        for dt in dts:
            sol.append(sol[-1] + (rk4_step(f, sol[-1], float(dt)) if method == "rk4" else float(dt) * f(sol[-1])))
        sol = torch.stack(sol)
    sol_leaf = sol.clone().requires_grad_(True)
    ro = lambda Y: torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(Y, Pt["linear3.weight"], Pt["linear3.bias"])),
                                              Pt["linearS2.weight"], Pt["linearS2.bias"])
    out = torch.softmax(torch.cat((ro(sol_leaf[:, :rows]), ro(sol_leaf[:, rows:2 * rows]), ro(sol_leaf[:, 2 * rows:3 * rows])), -1), 2)
    L = loss_of_outputs(out[..., 0], out[..., 1], out[..., 2])
    head = ["linear3.weight", "linear3.bias", "linearS2.weight", "linearS2.bias"]
    gr = torch.autograd.grad(L, [sol_leaf] + [Pt[k] for k in head])
    gsol = gr[0]
    grads = {k: g for k, g in zip(head, gr[1:])}
    Wd, bd = W.detach(), b.detach()

    def aug(state):
        y, a = state[0], state[1]
        fy, gy, gW, gb = rhs_vjp(y, Wd, bd, a, ridx, cidx)
        return (fy, -gy, -gW, -gb)

    a = gsol[-1].clone()
    gW, gb = torch.zeros_like(Wd), torch.zeros_like(bd)
    for i in range(sol.shape[0] - 1, 0, -1):
        h = -float(dts[i - 1])
        st = (sol[i], a, torch.zeros_like(Wd), torch.zeros_like(bd))
        if method == "rk4":
            F = lambda s: aug(s)
            add = lambda s, c, k: tuple(si + c * ki for si, ki in zip(s, k))
            third = 1.0 / 3.0
            k1 = F(st)
            k2 = F(add(st, h * third, k1))
            k3 = F(tuple(si + h * (b2 - b1 * third) for si, b1, b2 in zip(st, k1, k2)))
            k4 = F(tuple(si + h * (b1 - b2 + b3) for si, b1, b2, b3 in zip(st, k1, k2, k3)))
            inc = tuple((b1 + 3 * (b2 + b3) + b4) * h * 0.125 for b1, b2, b3, b4 in zip(k1, k2, k3, k4))
        else:
            inc = tuple(h * k for k in aug(st))
        a = a + inc[1] + gsol[i - 1]
        gW = gW + inc[2]
        gb = gb + inc[3]
    grads["odefunc.linear.weight"], grads["odefunc.linear.bias"] = gW, gb
    ge = torch.autograd.grad(y0, [Pt["linearS1.weight"], Pt["linearS1.bias"]], a)
    grads["linearS1.weight"], grads["linearS1.bias"] = ge
    return {k: v.detach().numpy().astype(np.float64) for k, v in grads.items()}


def l1_loss_of(y_labels, out_rows):
    """The reference's loss (ode_nn_ngraph_sim.py:230-234) over the outputs at grid rows `out_rows` (get_sir_t_nodes_torch):
    mean |pred - y| over [rows, T-1, 3], t = 0 excluded.  y_labels [rows, T, 3] float64."""
    yl = torch.from_numpy(np.asarray(y_labels, dtype=np.float64))
    idx = torch.as_tensor(np.asarray(out_rows), dtype=torch.int64)

    def L(S, I, R):
        pred = torch.stack((S[idx], I[idx], R[idx]), -1).transpose(0, 1)      # [rows, T, 3]
        return (pred[:, 1:, :] - yl.to(pred.dtype)[:, 1:, :]).abs().mean()
    return L
