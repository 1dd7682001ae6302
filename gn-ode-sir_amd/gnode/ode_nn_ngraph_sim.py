"""Drop-in for the model classes of reference ode_nn_ngraph_sim.py (the script
`model='ode_nn'` resolves to in monitorer-sim.py:26-33): same constructor
signatures, same state_dict key names, same forward shapes -- the arithmetic runs
in libgnode_hip.so on the MI355X.

    ODEfunc(A, beta, gamma, hidden1, device)            reference :37-96
    ODEBlock(maxTime, deltaT, n_nodes, indices, hidden1, odefunc, device)   :99-188
        (+ method="euler" | "rk4", adjoint=True | False: extensions)
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import autograd as _autograd
from . import ops
from .graph import DeviceGraph
from .ops import _check_adjoint  # noqa: F401  (the method / adjoint rule; imported from here by ode_nn_ngraphs and the tests)


def _rhs(func, graph, flat):
    """Both ODEfunc.forwards on flat [4*rows, H]: an autograd node when `func.differentiable` and grad is on, else the no_grad RHS."""
    if func.differentiable and torch.is_grad_enabled():
        return _autograd.rhs(graph, flat, func.linear.weight, func.linear.bias)
    with torch.no_grad():
        return ops.rhs(graph, flat, func.linear.weight, func.linear.bias)


class ODEfunc(nn.Module):
    def __init__(self, A, beta, gamma, hidden1, device, *, differentiable=False):
        super().__init__()
        # extension: differentiable=True makes forward an autograd node (gnode.autograd.rhs) whenever grad is enabled, so a
        # caller's own integrator (or torchdiffeq) can train through it; the default keeps the no_grad RHS
        self.differentiable = differentiable
        self.A = A
        self.beta = beta          # unused by forward, as in the reference (:42-43)
        self.gamma = gamma
        self.ln = nn.LayerNorm(hidden1)            # never applied in the reference (:94-95); kept for state_dict parity
        self.linear = nn.Linear(hidden1, hidden1)
        self.graph = DeviceGraph.from_scipy(A)     # CSR goes to HBM once, not once per RHS (:68-71)

    def init_weights(self):
        """reference :54-56 (defined, never called: the default nn.Linear init is what trains)."""
        nn.init.xavier_normal_(self.linear.weight)

    def forward(self, t, x):
        """x [4*B*n, H] -> dx (reference :58-96).  t is unused there too."""
        return _rhs(self, self.graph, x)


class _ODEBlock(nn.Module):
    """What the single-graph ODEBlock and gnode.ode_nn_ngraphs.ODEBlock share: the time grid, the sub-modules (created in the
    reference's order -- nn.Linear draws from the global RNG -- under the reference's state_dict keys) and the solve."""

    def __init__(self, maxTime, deltaT, hidden1, odefunc, device, method, adjoint):
        super().__init__()
        self.maxTime = maxTime
        self.deltaT = deltaT
        self.device = device
        self.method = method                        # the reference hard-codes 'euler' (:168)
        # extension: adjoint=False trains with the exact gradient of the Euler solve (torchdiffeq's odeint in place of
        # odeint_adjoint); the default is the reference's adjoint gradient
        self.adjoint = _check_adjoint(adjoint, method)
        self.integration_time = torch.from_numpy(ops.time_grid(maxTime, deltaT))
        self._dts = ops.step_sizes(ops.time_grid(maxTime, deltaT))
        self.odefunc = odefunc
        self.hidden1 = hidden1
        self.linearS1 = nn.Linear(1, hidden1)
        self.ln = nn.LayerNorm(hidden1)             # unused in the reference forward
        self.linear3 = nn.Linear(hidden1, 4)
        self.linearS2 = nn.Linear(4, 1)

    def _params(self):
        return {"odefunc.linear.weight": self.odefunc.linear.weight, "odefunc.linear.bias": self.odefunc.linear.bias,
                "linearS1.weight": self.linearS1.weight, "linearS1.bias": self.linearS1.bias,
                "linear3.weight": self.linear3.weight, "linear3.bias": self.linear3.bias,
                "linearS2.weight": self.linearS2.weight, "linearS2.bias": self.linearS2.bias}

    def _solve(self, graph, x2d, out_rows):
        """x2d [rows, 3+H] on `graph` -> (S, I, R), each [G, rows, 1]."""
        S, I, R = _autograd.forward_with_grad(graph, x2d, self._params(), self._dts, self.method, out_rows, self.adjoint)
        return S.unsqueeze(-1), I.unsqueeze(-1), R.unsqueeze(-1)


class ODEBlock(_ODEBlock):
    def __init__(self, maxTime, deltaT, n_nodes, indices, hidden1, odefunc, device, method="euler", adjoint=True):
        super().__init__(maxTime, deltaT, hidden1, odefunc, device, method, adjoint)
        self.n_nodes = n_nodes
        self.indices = torch.tensor(indices, requires_grad=False)

    def init_weights(self):
        """reference :139-146 (defined, never called)."""
        nn.init.kaiming_normal_(self.linearS1.weight, mode="fan_in", nonlinearity="relu")
        nn.init.kaiming_normal_(self.linear3.weight, mode="fan_in", nonlinearity="relu")
        self.linearS2.weight.data.normal_(0, 1)

    def forward(self, x, out_rows=None):
        """x [B, n, 3+H] -> (S, I, R), each [G, B*n, 1] (reference :148-188).

        out_rows (extension): ascending grid indices to emit instead of all G points;
        `ops.subsample_rows(maxTime, deltaT)` fuses get_sir_t_nodes_torch (ode_nn.py:249-261).
        """
        return self._solve(self.odefunc.graph, x.reshape(-1, x.size(-1)), out_rows)
