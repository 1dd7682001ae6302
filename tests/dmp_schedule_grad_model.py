"""The DMP recurrence under a rate schedule in torch with its gradients by autograd (a helper, not a test): the yardstick of
`gnode.dmp.dmp_marginals_schedule` and gnode_dmp_batch_schedule_backward_f32.

`forward` is tests/dmp_grad_model.py's `forward` with W [P, nnz], G [P, n] and `phase` [T] (entry 0 never read): step t reads
W[phase[t]] and G[phase[t]], and theta_{t+1} = theta_t - W[phase[t + 1]] phi_t reads the NEXT step's weight, as
csrc/gnode_dmp_schedule.hip does.  float32 is the restatement whose distance to float64 is the bar's `yard`, float64 the reference.
attribution="this" keeps the forward's numbers and sends theta_{t+1}'s weight gradient to step t's table instead: the mistake the
tests must be able to see.

The cases are tests/dmp_grad_model.py's `case(...)` with three phases: W = [w, 0.25 w, 0.6 w], G = [gam, min(2.5 gam, 1), 0.5 gam]
(float32 products), and `spread_phases(T)`: the steps 1 .. T-2 divided evenly among phases 0, 1, 2 and phase 0 again at the last
step; T = 2 is [-, 1] and T = 3 is [-, 1, 0]."""
import functools

import numpy as np

import dmp_grad_model as M


def forward(src, rev, n, W, G, phase, init, T, attribution="next"):
    """out [T, n, 3] = (Ps, Pi, Pr) from torch tensors W [P, nnz], G [P, n], init [n, 3] of one dtype; src, rev int64 tensors"""
    import torch
    dt = W.dtype
    one = torch.ones((), dtype=dt)
    ps0, pi0, pr0 = init[:, 0], init[:, 1], init[:, 2]

    def row_product(theta):                                     # CPU scatter: sequential, so ascending position within a row
        return torch.ones(n, dtype=dt).scatter_reduce(0, src, theta[rev], "prod", include_self=True)

    theta = (one - W[int(phase[1])] * pi0[src]) + torch.tensor(1e-10, dtype=dt)
    phi, q = pi0[src], ps0[src]
    Pi, Pr = pi0, pr0
    out = [init]
    for t in range(1, T):
        w, gamma = W[int(phase[t])], G[int(phase[t])]
        P = row_product(theta)
        Ps = ps0 * P
        Pr = Pr + gamma * Pi
        Pi = one - Ps - Pr
        out.append(torch.stack([Ps, Pi, Pr], 1))
        if t + 1 < T:
            q_new = ps0[src] * (P[src] / theta[rev])
            phi = (one - w) * (one - gamma[src]) * phi - (q_new - q)
            q = q_new
            w_next = W[int(phase[t + 1])]
            if attribution == "this":                           # the next step's value, this step's table's gradient
                w_next = w_next.detach() + (w - w.detach())
            theta = theta - w_next * phi
    return torch.stack(out, 0)


def gradients(rp, ci, W, G, phase, init, T, grad_out, dtype="float64", attribution="next"):
    """(out, grad_W [P, nnz], grad_G [P, n], grad_init) as numpy arrays of `dtype`: the vector-Jacobian product with grad_out"""
    import torch
    dt = getattr(torch, dtype)
    src, rev = (torch.from_numpy(a) for a in M.tables(rp, ci))
    leaves = [torch.tensor(np.asarray(a, dtype=np.float64), dtype=dt, requires_grad=True) for a in (W, G, init)]
    out = forward(src, rev, len(rp) - 1, leaves[0], leaves[1], phase, leaves[2], T, attribution)
    out.backward(torch.tensor(np.asarray(grad_out, dtype=np.float64), dtype=dt))
    return (out.detach().numpy(), *(np.zeros(x.shape, dtype) if x.grad is None else x.grad.numpy() for x in leaves))


# --------------------------------------------------------------------------------------------------------------- cases
def spread_phases(T, P=3):
    """int32 [T]: steps 1 .. T-2 divided evenly among the phases 0 .. P-1 in order, phase 0 revisited at step T-1"""
    if T <= 3:
        return np.asarray([0, 1, 0][:T], dtype=np.int32)
    phase = np.zeros(T, dtype=np.int32)
    phase[1:T - 1] = (np.arange(T - 2) * P) // (T - 2)
    return phase


def three_tables(w, gam):
    """W [3, nnz], G [3, n], float32"""
    w, gam = np.asarray(w, np.float32), np.asarray(gam, np.float32)
    W = np.stack([w, w * np.float32(0.25), w * np.float32(0.6)]).astype(np.float32)
    G = np.stack([gam, np.minimum(gam * np.float32(2.5), np.float32(1.0)), gam * np.float32(0.5)]).astype(np.float32)
    return W, G


@functools.lru_cache(maxsize=None)
def case(name, start="mixed"):
    """dmp_grad_model.case(name, start) with W [3, nnz], G [3, n] and phase [T] added; read-only"""
    c = dict(M.case(name, start))
    c["W"], c["Gam"] = three_tables(c["w"], c["gam"])
    c["phase"] = spread_phases(c["T"])
    for key in ("W", "Gam", "phase"):
        c[key].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def model(name, start="mixed", dtype="float64"):
    """`gradients` of a named case, once per (case, start, dtype); the arrays are read-only"""
    c = case(name, start)
    res = gradients(c["rp"], c["ci"], c["W"], c["Gam"], c["phase"], c["init"], c["T"], c["G"], dtype)
    for a in res:
        a.setflags(write=False)
    return res
