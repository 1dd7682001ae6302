"""float64 torch restatement of the GN-ODE model and of its gradients  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Every GPU gradient the library returns is held to this module, and this module is held to fixtures the reference's own
classes produced (tests/golden/*.npz): the RHS vector-Jacobian product (rhs_vjp_*), the Euler and RK4 adjoints (adjoint_*,
rk4_adjoint_*, real_*, input_grad_*) and the exact gradient of the Euler solve (discrete_*).

  * ``rhs_vjp`` is written out from the spec's formulas, not taken by autograd: the fixtures are autograd
    through the reference's ODEfunc, so agreement checks the formulas the kernels implement.
  * ``adjoint`` restates torchdiffeq 0.2.2's odeint_adjoint for method 'euler' and 'rk4' (3/8 rule) -- parity-unpinned,
    like the Euler rule of SURVEY Appendix A: torchdiffeq is absent.
  * ``exact_grads`` is torch autograd through a plain Euler loop -- exact by construction.

Inputs are numpy (float32 as the library takes them); every function that converts them has a ``dtype`` argument, float64
by default.  A graph is ``(rowptr, col)``: B samples of one graph, or one sample over a concatenated multi-graph CSR
(gnode_oracle.concat_csr); the state's row count says which.
"""
from __future__ import annotations

import numpy as np
import torch

KEYS = ("odefunc.linear.weight", "odefunc.linear.bias", "linearS1.weight", "linearS1.bias",
        "linear3.weight", "linear3.bias", "linearS2.weight", "linearS2.bias")
F64 = torch.float64


# --------------------------------------------------------------------------- graph indexing and the RHS
def index(rowptr, col, rows):
    """(ridx, cidx) of the block-diagonal CSR over the rows // n samples of the n-node graph (rowptr, col)."""
    n = len(rowptr) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    dst = np.asarray(col, dtype=np.int64)
    B = rows // n
    ridx = torch.from_numpy(np.concatenate([src + b * n for b in range(B)]))
    cidx = torch.from_numpy(np.concatenate([dst + b * n for b in range(B)]))
    return ridx, cidx


def _spmm(ridx, cidx, T):
    return torch.zeros_like(T).index_add(0, ridx, T[cidx])


def rhs(y, W, b, ridx, cidx):
    """ODEfunc.forward (ode_nn_ngraph_sim.py:58-96) on torch tensors: y [4*q, H] -> dy/dt."""
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
    """(f, v^T df/dy, v^T df/dW, v^T df/db) from the formulas (A symmetric).  The beta-gamma slab of v^T df/dy is
        d/dbeta = sum_h (v_I - v_S) AI Z_S        d/dgamma = sum_h (v_R - v_I) Z_I        (AI = A Z_I)
    in its columns 0 and 1, and 0 elsewhere."""
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


def rhs_vjp_np(y, W, b, v, rowptr, col, dtype=F64):
    """rhs_vjp on numpy inputs: (f, gy, gW, gb) as numpy."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    ridx, cidx = index(rowptr, col, y.shape[0] // 4)
    return tuple(o.numpy() for o in rhs_vjp(t(y), t(W), t(b), t(v), ridx, cidx))


# --------------------------------------------------------------------------- integrators
def rk4_step(f, y, dt):
    """torchdiffeq 0.2.2 rk4_alt_step_func (3/8 rule): the increment of one step of size dt."""
    third = 1.0 / 3.0
    k1 = f(y)
    k2 = f(y + dt * k1 * third)
    k3 = f(y + dt * (k2 - k1 * third))
    k4 = f(y + dt * (k1 - k2 + k3))
    return (k1 + 3 * (k2 + k3) + k4) * dt * 0.125


def _increment(f, y, dt, method):
    return rk4_step(f, y, dt) if method == "rk4" else dt * f(y)


def _widen(dts):
    """the fp32 step sizes the library integrates with, as float64 numbers"""
    return np.asarray(dts, dtype=np.float32).astype(np.float64)


def trajectory(y0, W, b, ridx, cidx, dts, method="euler"):
    """sol [G, 4*q, H]: y0 and the state after each step of size dts[k] ('euler' or 'rk4')."""
    f = lambda y: rhs(y, W, b, ridx, cidx)
    sol = [y0]
    for dt in _widen(dts):
        sol.append(sol[-1] + _increment(f, sol[-1], float(dt), method))
    return torch.stack(sol)


# --------------------------------------------------------------------------- encoder and read-out head
def encode(x2, Pt):
    """y0 [4*rows, H] of x2 [rows, 3+H]: relu(Linear(1, H)) of S0, I0, R0, then the beta-gamma slab (ode_nn_ngraph_sim.py:151-156)."""
    enc = lambda s: torch.relu(torch.nn.functional.linear(s.unsqueeze(-1), Pt["linearS1.weight"], Pt["linearS1.bias"]))
    return torch.cat((enc(x2[:, 0]), enc(x2[:, 1]), enc(x2[:, 2]), x2[:, 3:]))


def head(sol, Pt):
    """(S, I, R), each [G, rows]: Linear(4, 1)(relu(Linear(H, 4))) of each compartment, softmax across the three
    (ode_nn_ngraph_sim.py:172-187)."""
    q = sol.shape[1] // 4
    ro = lambda Y: torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(Y, Pt["linear3.weight"], Pt["linear3.bias"])),
                                              Pt["linearS2.weight"], Pt["linearS2.bias"])
    out = torch.softmax(torch.cat((ro(sol[:, :q]), ro(sol[:, q:2 * q]), ro(sol[:, 2 * q:3 * q])), -1), 2)
    return out[..., 0], out[..., 1], out[..., 2]


def _setup(x2d, P, graph, dtype):
    """(P, x2d as leaves that require grad, ridx, cidx)"""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(True)
    Pt = {k: t(v) for k, v in P.items()}
    x2 = t(x2d)
    return (Pt, x2) + index(*graph, x2.shape[0])


def _numpy(grads):
    return {k: g.detach().numpy() for k, g in grads.items()}


# --------------------------------------------------------------------------- the loss and its gradients
def forward_loss(x2d, P, graph, dts, loss_of_outputs, method="euler", dtype=F64):
    """loss_of_outputs(S, I, R) of the forward, as a Python float."""
    with torch.no_grad():
        Pt, x2, ridx, cidx = _setup(x2d, P, graph, dtype)
        sol = trajectory(encode(x2, Pt), Pt["odefunc.linear.weight"], Pt["odefunc.linear.bias"], ridx, cidx, dts, method)
        return float(loss_of_outputs(*head(sol, Pt)))


def adjoint(x2d, P, graph, dts, loss_of_outputs, method="euler", stop_at=1, dtype=F64):
    """{the 8 parameter gradients, "x": dL/dx2d [rows, 3+H]} as numpy for L = loss_of_outputs(S, I, R) (each [G, rows] torch)
    under torchdiffeq 0.2.2's odeint_adjoint: the forward on the grid under no_grad, sol saved; the head's VJP by autograd on
    sol; a <- dL/dsol[G-1]; then per interval i = G-1 .. stop_at one step of size -dt_{i-1} ('euler' or 'rk4', as the
    forward) of the augmented system (y, a, g_W, g_b)' = (f, -a^T df/dy, -a^T df/dW, -a^T df/db) from (sol[i], a, 0, 0),
    its a and g increments kept, y reset to sol[i-1] and dL/dsol[i-1] added to a; finally a flows into the encoder.  "x" is
    therefore the encoder's relu-masked VJP in columns 0-2, the beta-gamma slab's adjoint in columns 3-4 and 0 elsewhere.
    stop_at > 1 ends the sweep early (intervals below stop_at are skipped): a deliberately wrong rule for sensitivity checks."""
    Pt, x2, ridx, cidx = _setup(x2d, P, graph, dtype)
    W, b = Pt["odefunc.linear.weight"].detach(), Pt["odefunc.linear.bias"].detach()
    y0 = encode(x2, Pt)
    with torch.no_grad():
        sol = trajectory(y0.detach(), W, b, ridx, cidx, dts, method)
    sol_leaf = sol.clone().requires_grad_(True)
    gsol, *grads = torch.autograd.grad(loss_of_outputs(*head(sol_leaf, Pt)), [sol_leaf] + [Pt[k] for k in KEYS[4:]])
    # the augmented state as one flat tensor, so that the forward's step rule takes it as it is
    m, nW = y0.numel(), W.numel()

    def aug(s):
        f, gy, gW, gb = rhs_vjp(s[:m].view_as(y0), W, b, s[m:2 * m].view_as(y0), ridx, cidx)
        return torch.cat((f.ravel(), -gy.ravel(), -gW.ravel(), -gb.ravel()))

    a, gW, gb = gsol[-1], torch.zeros_like(W), torch.zeros_like(b)
    zero_g = torch.zeros(nW + b.numel(), dtype=dtype)
    dts = _widen(dts)
    for i in range(len(dts), stop_at - 1, -1):
        inc = _increment(aug, torch.cat((sol[i].ravel(), a.ravel(), zero_g)), -float(dts[i - 1]), method)
        a = a + inc[m:2 * m].view_as(a) + gsol[i - 1]
        gW = gW + inc[2 * m:2 * m + nW].view_as(W)
        gb = gb + inc[2 * m + nW:]
    grads += [gW, gb] + list(torch.autograd.grad(y0, [Pt["linearS1.weight"], Pt["linearS1.bias"], x2], a))
    return _numpy(dict(zip(KEYS[4:] + KEYS[:4] + ("x",), grads)))


def exact_grads(x2d, P, graph, dts, loss_of_outputs, dtype=F64):
    """adjoint's dict for the exact gradient of the Euler solve y_k = y_{k-1} + dt_{k-1} f(y_{k-1}): autograd through the
    loop (include/gnode.h gnode_backward_discrete_f32)."""
    Pt, x2, ridx, cidx = _setup(x2d, P, graph, dtype)
    sol = trajectory(encode(x2, Pt), Pt["odefunc.linear.weight"], Pt["odefunc.linear.bias"], ridx, cidx, dts, "euler")
    grads = torch.autograd.grad(loss_of_outputs(*head(sol, Pt)), [Pt[k] for k in KEYS] + [x2])
    return _numpy(dict(zip(KEYS + ("x",), grads)))


# --------------------------------------------------------------------------- losses
def l1_loss_of(y_labels, out_rows):
    """The reference's loss (ode_nn_ngraph_sim.py:230-234) over the outputs at grid rows `out_rows` (get_sir_t_nodes_torch):
    mean |pred - y| over [rows, T-1, 3], t = 0 excluded.  y_labels [rows, T, 3] float64."""
    yl = torch.from_numpy(np.asarray(y_labels, dtype=np.float64))
    idx = torch.as_tensor(np.asarray(out_rows), dtype=torch.int64)

    def L(S, I, R):
        pred = torch.stack((S[idx], I[idx], R[idx]), -1).transpose(0, 1)      # [rows, T, 3]
        return (pred[:, 1:, :] - yl.to(pred.dtype)[:, 1:, :]).abs().mean()
    return L


def linear_loss(gS, gI, gR, out_rows=None):
    """sum(gS * S[out_rows]) + ...: the loss whose upstream gradients are gS, gI, gR ([n_out, rows] numpy)"""
    g = [torch.from_numpy(np.asarray(a, dtype=np.float64)) for a in (gS, gI, gR)]
    idx = None if out_rows is None else torch.as_tensor(np.asarray(out_rows), dtype=torch.int64)

    def L(S, I, R):
        pick = (lambda A: A) if idx is None else (lambda A: A[idx])
        return sum((pick(A) * gA.to(A.dtype)).sum() for A, gA in zip((S, I, R), g))
    return L
