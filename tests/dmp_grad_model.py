"""The DMP recurrence in torch with its gradients by autograd (a helper, not a test): the yardstick of the differentiable DMP
baseline (`gnode.dmp.dmp_marginals`, gnode_dmp_batch_backward_f32).

`forward` states the recurrence as csrc/gnode_dmp.hip does -- theta_1 = (1 - w Pi_0[src]) + 1e-10, P_k the product of
theta[rev(e)] over row k in ascending position, the cavity product as P[src] / theta[rev], Pr before Pi -- in the dtype asked for:
float32 is the restatement whose distance to float64 is the bar's `yard`, float64 the reference.  `gradients` runs it with
autograd for a given grad_out.  The case builders reuse the graphs, weights and gammas of tests/baseline_cases.py; the starts
are one-hot seeds or mixed states from default_rng(seed).dirichlet([4, .5, .5], n), grad_out is default_rng(0).standard_normal,
and no case has a weight of 1 (theta = 0 next to a seed: the forward is not finite there and the gradient is unspecified)."""
import functools

import numpy as np

from baseline_cases import DMP_CASES, gammas, weights


def tables(rp, ci):
    """(src, rev) of a symmetric CSR pattern, int64: the row of each position and the position of its reverse edge."""
    from sir_init_model import dmp_reverse_index
    src = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    rev = np.asarray(dmp_reverse_index(rp, ci), dtype=np.int64)
    assert len(ci) == 0 or rev.max() < len(ci), "the pattern is not symmetric"
    return src, rev


def forward(src, rev, n, w, gamma, init, T):
    """out [T, n, 3] = (Ps, Pi, Pr) from torch tensors w [nnz], gamma [n], init [n, 3] of one dtype; src, rev int64 tensors."""
    import torch
    dt = w.dtype
    one = torch.ones((), dtype=dt)
    ps0, pi0, pr0 = init[:, 0], init[:, 1], init[:, 2]

    def row_product(theta):                                     # CPU scatter: sequential, so ascending position within a row
        return torch.ones(n, dtype=dt).scatter_reduce(0, src, theta[rev], "prod", include_self=True)

    theta = (one - w * pi0[src]) + torch.tensor(1e-10, dtype=dt)
    phi, q = pi0[src], ps0[src]
    Pi, Pr = pi0, pr0
    out = [init]
    for t in range(1, T):
        P = row_product(theta)
        Ps = ps0 * P
        Pr = Pr + gamma * Pi
        Pi = one - Ps - Pr
        out.append(torch.stack([Ps, Pi, Pr], 1))
        if t + 1 < T:
            q_new = ps0[src] * (P[src] / theta[rev])
            phi = (one - w) * (one - gamma[src]) * phi - (q_new - q)
            q = q_new
            theta = theta - w * phi
    return torch.stack(out, 0)


def gradients(rp, ci, w, gamma, init, T, grad_out, dtype="float64"):
    """(out, grad_w, grad_gamma, grad_init) as numpy arrays of `dtype`: the vector-Jacobian product of `forward` with grad_out."""
    import torch
    dt = getattr(torch, dtype)
    src, rev = (torch.from_numpy(a) for a in tables(rp, ci))
    leaves = [torch.tensor(np.asarray(a, dtype=np.float64), dtype=dt, requires_grad=True) for a in (w, gamma, init)]
    out = forward(src, rev, len(rp) - 1, *leaves, T)
    out.backward(torch.tensor(np.asarray(grad_out, dtype=np.float64), dtype=dt))
    return (out.detach().numpy(), *(np.zeros(x.shape, dtype) if x.grad is None else x.grad.numpy() for x in leaves))


# --------------------------------------------------------------------------------------------------------------- cases
def seed_state(n, seeds):
    p = np.zeros((n, 3), dtype=np.float32)
    p[:, 0] = 1.0
    p[list(seeds)] = (0.0, 1.0, 0.0)
    return p


def mixed_state(n, seed):
    return np.random.default_rng(seed).dirichlet([4, .5, .5], n).astype(np.float32)


def grad_out_of(T, n, B=None):
    shape = (T, n, 3) if B is None else (B, T, n, 3)
    return np.random.default_rng(0).standard_normal(shape).astype(np.float32)


def _horizon8():
    c = DMP_CASES["T3"]()
    return dict(c, T=8)


def _w0_gamma01():
    c = DMP_CASES["w_zero"]()                                   # a third of the weights 0 ...
    return dict(c, gam=DMP_CASES["gamma_01"]()["gam"])          # ... and gamma at 0 and at 1


GRAPHS = {"er300_T2": DMP_CASES["T2"], "er300_T3": DMP_CASES["T3"], "er300_T8": _horizon8, "er34": _w0_gamma01,
          "isolated": DMP_CASES["isolated"], "nnz0": DMP_CASES["nnz0"], "hub": DMP_CASES["hub"]}
START_SEED = {name: 40 + i for i, name in enumerate(GRAPHS)}


@functools.lru_cache(maxsize=None)
def case(name, start="mixed"):
    """dict(rp, ci, w, gam, init, T, G) of a named case, float32 inputs, read-only; start: "mixed" or "seeds"."""
    c = GRAPHS[name]()
    n = len(c["rp"]) - 1
    assert not (np.asarray(c["w"]) == 1.0).any()
    init = mixed_state(n, START_SEED[name]) if start == "mixed" else seed_state(n, c["seeds"])
    out = dict(rp=c["rp"], ci=c["ci"], w=np.asarray(c["w"], np.float32), gam=np.asarray(c["gam"], np.float32), init=init, T=c["T"],
               G=grad_out_of(c["T"], n))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model(name, start="mixed", dtype="float64"):
    """`gradients` of a named case, once per (case, start, dtype); the arrays are read-only."""
    c = case(name, start)
    res = gradients(c["rp"], c["ci"], c["w"], c["gam"], c["init"], c["T"], c["G"], dtype)
    for a in res:
        a.setflags(write=False)
    return res


__all__ = ["case", "forward", "gradients", "gammas", "grad_out_of", "mixed_state", "model", "seed_state", "tables", "weights"]
