"""Drop-in for the helpers of reference ode_nn.py that sit on the hot path:

    sir_torch(G, seed_set, beta, gamma, sims=10000, T=20)        reference :30-88
    rate_schedule(values, starts=None, steps=None)               extension: a rate that changes over time, for the
                                                                 Monte-Carlo calls here and gnode.dmp.dmp_batch
    get_sir_t_nodes_torch(x_rk, maxTime, deltaT, count=True)     reference :249-261
    create_graph(n_nodes, graph_label='none')                    reference :394-414
    sir(x, y, A, beta, gamma), runge_kutta_order4(sir, A, ...)   reference :214-233 (mean-field comparison column)
    meanfield_batch(graph, starts, beta, gamma, ...)             extension: that column for a batch of samples
    meanfield_marginals(graph, init, beta, gamma, w, ...)        extension: the same numbers as a differentiable function
"""
from __future__ import annotations

import ctypes as C
import math
import os
import pickle
from typing import NamedTuple

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from .graph import DeviceGraph


def _edge_arrays(G):
    if hasattr(G, "edge_array"):                      # CsrGraph (restored from the CSR cache file)
        return G.edge_array
    e = np.asarray(list(G.edges()), dtype=np.int64).reshape(-1, 2)
    return e


def _csr_from_edges(n, e):
    r = np.concatenate([e[:, 0], e[:, 1]])
    c = np.concatenate([e[:, 1], e[:, 0]])
    a = sp.coo_matrix((np.ones(r.shape[0], dtype=np.int8), (r, c)), shape=(n, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32)


_GRAPH_CACHE: dict = {}


def _device_graph_for(G):
    """The label loop calls sir_torch once per (seed set, beta, gamma) on the SAME networkx graph
    (ode_nn_ngraph_sim.py:360-368): build and upload its CSR once, not 200 times."""
    import weakref
    key = (id(G), G.number_of_nodes(), G.number_of_edges())
    hit = _GRAPH_CACHE.get(key)
    if hit is not None and hit[0]() is G:            # same live object, not a recycled id
        return hit[1]
    if len(_GRAPH_CACHE) >= 4:
        _GRAPH_CACHE.pop(next(iter(_GRAPH_CACHE)))
    dg = DeviceGraph(*_csr_from_edges(G.number_of_nodes(), _edge_arrays(G)))
    try:
        _GRAPH_CACHE[key] = (weakref.ref(G), dg)
    except TypeError:                                # not weak-referenceable: do not cache
        pass
    return dg


def _node_rates(name: str, value, n: int):
    """None when `value` is a scalar rate; else the validated per-node rates as a contiguous float64 [n] host array
    (from a numpy array, a list or a torch tensor on any device).  Raises ValueError before any library call."""
    if isinstance(value, torch.Tensor):
        if value.ndim == 0:
            return None
        value = value.detach().cpu().numpy()
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0:
        return None
    if a.shape != (n,):
        raise ValueError(f"{name}: per-node rates must have shape ({n},), got {tuple(a.shape)}")
    bad = np.flatnonzero(~((a >= 0.0) & (a <= 1.0)))            # a NaN fails both comparisons
    if bad.size:
        raise ValueError(f"{name}[{int(bad[0])}] = {a[bad[0]]} is not a probability in [0, 1]")
    return np.ascontiguousarray(a)


class EdgeRates:
    """Per-edge transmission probabilities for `sir_counts` / `sir_trajectories` / `sir_torch` (pass it as `beta`): `w`, a
    validated contiguous float64 [nnz] host array in the CSR position order of the graph it was made for (n nodes).  w[p] is
    the probability per step that the row of position p infects col[p].  Made by `edge_rates`."""

    def __init__(self, w: np.ndarray, n: int):
        self.w, self.n, self.nnz = w, int(n), int(w.shape[0])


def _host_csr(graph):
    """(n, rowptr, col) on the host of a DeviceGraph, a networkx graph (the CSR sir_torch builds for it) or a (rowptr, col) pair."""
    if hasattr(graph, "number_of_nodes"):
        rp, ci = _csr_from_edges(graph.number_of_nodes(), _edge_arrays(graph))
    elif isinstance(graph, (tuple, list)):
        rp, ci = graph
    else:
        rp, ci = graph.rowptr, graph.col
    rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    return int(rp.shape[0] - 1), rp, ci


def edge_rates(graph, M) -> EdgeRates:
    """Per-edge transmission probabilities in the graph's CSR position order, for `beta` of the Monte-Carlo calls.

    graph: a DeviceGraph, a networkx graph, or a (rowptr, col) pair.  M: an array of length nnz already in CSR position
    order, or a scipy sparse [n, n] matrix with M[u, v] = the probability per step that the infected u infects the
    susceptible v (source = row, target = column: what `DMP_SIR` takes as `weight_adj`, so one matrix serves both).
    Entries of the pattern that M does not store are 0: the graph's pattern is symmetric, and a directed contact u -> v is
    M[u, v] > 0 with M[v, u] absent or 0.  Raises ValueError for a wrong shape, a NaN, a value outside [0, 1] and a
    non-zero entry of M outside the pattern."""
    n, rp, ci = _host_csr(graph)
    nnz = int(ci.shape[0])
    if sp.issparse(M):
        if M.shape != (n, n):
            raise ValueError(f"edge_rates: the matrix must have shape ({n}, {n}), got {tuple(M.shape)}")
        m = sp.coo_matrix(M, dtype=np.float64)
        m.sum_duplicates()
        keep = m.data != 0.0                                        # (a NaN is kept: it is not an absent entry)
        mr, mc, mv = m.row[keep].astype(np.int64), m.col[keep].astype(np.int64), m.data[keep]
        key = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp)) * n + ci        # of every CSR position
        order = np.argsort(key, kind="stable")
        at = np.searchsorted(key[order], mr * n + mc)
        hit = at < nnz
        hit[hit] = key[order][at[hit]] == (mr * n + mc)[hit]
        if not hit.all():
            k = int(np.flatnonzero(~hit)[0])
            raise ValueError(f"edge_rates: M[{int(mr[k])}, {int(mc[k])}] = {mv[k]} lies outside the graph's pattern")
        w = np.zeros(nnz, dtype=np.float64)
        w[order[at]] = mv
    else:
        if isinstance(M, torch.Tensor):
            M = M.detach().cpu().numpy()
        w = np.array(M, dtype=np.float64)
        if w.shape != (nnz,):
            raise ValueError(f"edge_rates: per-edge rates must have shape ({nnz},), got {tuple(w.shape)}")
    bad = np.flatnonzero(~((w >= 0.0) & (w <= 1.0)))                # a NaN fails both comparisons
    if bad.size:
        raise ValueError(f"edge_rates: the rate at CSR position {int(bad[0])}, {w[bad[0]]}, is not a probability in [0, 1]")
    return EdgeRates(np.ascontiguousarray(w), n)


def _edge_rate_args(er: EdgeRates, gamma, graph):
    """The rate arguments of the gnode_sir_mc_philox*_edges entries -- (w, gamma, gamma_host) -- and the host array to keep
    alive; raises ValueError when `er` was made for another graph or gamma is not a rate."""
    if (er.n, er.nnz) != (graph.n, graph.nnz):
        raise ValueError(f"EdgeRates of a graph with {er.n} nodes / {er.nnz} entries given for one with {graph.n} / {graph.nnz}")
    g = _node_rates("gamma", gamma, graph.n)
    if g is None:
        _node_rates("gamma", np.full(1, float(gamma)), 1)           # the scalar, through the same check
        return (_lib.host_ptr(er.w), float(gamma), None), g
    return (_lib.host_ptr(er.w), 0.0, _lib.host_ptr(g)), g


class InitialState:
    """An initial-state distribution for the label generators and baselines, passed wherever a seed set goes (`sir_counts`,
    `sir_trajectories`, `sir_torch`, `DMP_SIR.run`, `runge_kutta_order4`): `p`, a validated contiguous float64 [n, 3] host
    array of (pS, pI, pR) per node -- the GN-ODE's own x[:, 0:3].  The Monte-Carlo draws every trajectory's start from it,
    independently per node; DMP and the mean-field start from it as it is.  Made by `initial_state` or `from_sets`."""

    def __init__(self, p: np.ndarray):
        self.p, self.n = p, int(p.shape[0])

    @classmethod
    def from_sets(cls, n: int, infected, immune=()) -> "InitialState":
        """The crisp state: `infected` nodes start in I, `immune` nodes in R (vaccinated), everybody else in S."""
        p = np.zeros((int(n), 3), dtype=np.float64)
        p[:, 0] = 1.0
        for ids, c in ((infected, 1), (immune, 2)):
            ids = np.asarray(list(ids), dtype=np.int64)
            if ids.size and (ids.min() < 0 or ids.max() >= n):
                raise ValueError(f"InitialState.from_sets: node {int(ids[(ids < 0) | (ids >= n)][0])} is not in [0, {n})")
            if ids.size and p[ids, 0].min() == 0.0:
                raise ValueError("InitialState.from_sets: a node is both infected and immune")
            p[ids, 0], p[ids, c] = 0.0, 1.0
        return initial_state(p)

    def x(self, hidden: int, beta, gamma) -> torch.Tensor:
        """The float32 [n, 3 + hidden] sample `trainer.sample_tensor` would build, columns 0..2 taken from `p`."""
        x = torch.zeros(self.n, 3 + int(hidden), dtype=torch.float32)
        x[:, :3] = torch.from_numpy(self.p).to(torch.float32)
        x[:, 3] = torch.as_tensor(beta, dtype=torch.float32)
        x[:, 4] = torch.as_tensor(gamma, dtype=torch.float32)
        return x


def initial_state(p) -> InitialState:
    """An `InitialState` from an [n, 3] array-like of (pS, pI, pR) per node (numpy, list or torch tensor on any device;
    x[:, :3] of a sample works).  The checks of gnode_sir_mc_philox_init, raised as ValueError before the library is
    entered: the shape, a NaN, an entry outside [0, 1], a row whose sum is off 1 by more than 1e-6.  Nothing is renormalised."""
    if isinstance(p, torch.Tensor):
        p = p.detach().cpu().numpy()
    a = np.array(p, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"initial_state: need (pS, pI, pR) per node, shape [n, 3], got {tuple(a.shape)}")
    bad = np.argwhere(~((a >= 0.0) & (a <= 1.0)))                   # a NaN fails both comparisons
    if bad.size:
        v, c = int(bad[0][0]), int(bad[0][1])
        raise ValueError(f"initial_state: p[{v}][{c}] = {a[v, c]} is not a probability in [0, 1]")
    off = np.flatnonzero(~(np.abs(a[:, 0] + a[:, 1] + a[:, 2] - 1.0) <= 1e-6))
    if off.size:
        raise ValueError(f"initial_state: the row of node {int(off[0])} sums to {a[off[0]].sum()!r}, not 1")
    return InitialState(np.ascontiguousarray(a))


class RateSchedule:
    """A rate that changes over time, piecewise constant: `values`, P >= 1 of whatever the argument it replaces accepts as a
    constant, and which of them governs each step.  A call over T grid points takes steps t = 1 .. T-1, step t leading from
    state t-1 to state t.  Made by `rate_schedule`; pass it as `beta` / `gamma` of `sir_counts`, `sir_trajectories` and
    `sir_torch`, or as `weight_adj` / `scale` / `gamma` of `gnode.dmp.dmp_batch`."""

    def __init__(self, values, starts, steps):
        self.values, self.P, self.starts, self.steps = values, len(values), starts, steps

    def phase_of_step(self, T) -> np.ndarray:
        """int32 [T]: entry t is the index of the value that governs step t; entry 0 is 0 and is never read.  ValueError when
        the schedule was given as `steps` and holds fewer than T entries."""
        T = int(T)
        if T < 1:
            raise ValueError(f"RateSchedule.phase_of_step: T must be >= 1 (got {T})")
        out = np.zeros(T, dtype=np.int32)
        if self.steps is not None:
            if T > self.steps.shape[0]:
                raise ValueError(f"RateSchedule: the schedule names {self.steps.shape[0]} steps, the call has T = {T}")
            out[1:] = self.steps[1:T]
        else:
            out[1:] = np.searchsorted(self.starts, np.arange(1, T), side="right") - 1
        return out


def _whole_numbers(who, name, value):
    """`value` as a 1-D int64 array of whole numbers; ValueError otherwise."""
    try:
        a = np.asarray(value)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu" and not (a.dtype.kind == "f" and (np.isfinite(a) & (a == np.floor(a))).all())):
            raise ValueError("not a sequence of whole numbers")
        return a.astype(np.int64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{who}: {name} is not a sequence of whole numbers ({e})") from None


def rate_schedule(values, starts=None, steps=None) -> RateSchedule:
    """A piecewise-constant schedule of P >= 1 values for a rate argument (see `RateSchedule`).

    values: each one whatever the argument it replaces accepts as a constant (checked by the call that takes the schedule).
    Give exactly one of
      starts: P ascending whole numbers with starts[0] == 1; value p holds for steps starts[p] .. starts[p+1] - 1, the last to
              the end.  Starts at or beyond a call's T are ignored.
      steps:  a sequence with steps[t] in [0, P) for t >= 1 (entry 0 is ignored): periodic patterns, phases revisited.  A
              call's T must not exceed its length.
    What is wrong raises ValueError."""
    who = "rate_schedule"
    if isinstance(values, (RateSchedule, EdgeRates, str)) or not hasattr(values, "__len__"):
        raise ValueError(f"{who}: values must be a sequence of P >= 1 values")
    values = list(values)
    P = len(values)
    if P < 1:
        raise ValueError(f"{who}: values must hold at least one value")
    if any(isinstance(v, RateSchedule) for v in values):
        raise ValueError(f"{who}: a value cannot be a schedule itself")
    if (starts is None) == (steps is None):
        raise ValueError(f"{who}: give exactly one of starts and steps")
    if starts is not None:
        st = _whole_numbers(who, "starts", starts)
        if st.shape[0] != P:
            raise ValueError(f"{who}: {P} values need {P} starts, got {st.shape[0]}")
        if st[0] != 1 or (np.diff(st) <= 0).any():
            raise ValueError(f"{who}: starts must ascend from starts[0] == 1, got {st.tolist()}")
        return RateSchedule(values, st, None)
    sp_ = _whole_numbers(who, "steps", steps)
    if sp_.shape[0] < 1:
        raise ValueError(f"{who}: steps must hold at least one entry")
    bad = np.flatnonzero((sp_[1:] < 0) | (sp_[1:] >= P))
    if bad.size:
        raise ValueError(f"{who}: steps[{int(bad[0]) + 1}] = {int(sp_[bad[0] + 1])} is not in [0, {P})")
    return RateSchedule(values, None, sp_)


def refuse_schedule(who, **args):
    """ValueError when one of the named arguments is a `RateSchedule`: the calls that take constant rates only."""
    for name, v in args.items():
        if isinstance(v, RateSchedule):
            raise ValueError(f"{who}: {name} is a RateSchedule; this call takes constant rates "
                             "(schedules: sir_counts, sir_trajectories, sir_torch, dmp_batch; gradients under one: dmp_marginals_schedule; source "
                             "scores and outbreak sizes under one: source_scores_schedule, outbreak_sizes_schedule)")


def joint_phases(phases):
    """The joint schedule of several per-step phase rows (int [T] each): (phase int32 [T], tuples), tuples[j] = the combination
    of the rows' phases that joint phase j stands for -- the distinct combinations over steps 1 .. T-1 in order of first use
    (for T = 1, the one combination of entry 0)."""
    rows = np.stack([np.asarray(p, dtype=np.int64) for p in phases], axis=1)
    T = rows.shape[0]
    index, phase = {}, np.zeros(T, dtype=np.int32)
    for t in (range(1, T) if T > 1 else range(1)):
        phase[t] = index.setdefault(tuple(int(x) for x in rows[t]), len(index))
    return phase, list(index)


class _SirSchedule:
    """The checked host side of a scheduled Monte-Carlo call: phase int32 [T], W float64 [P, nnz], G float64 [P, n]."""

    def __init__(self, phase, W, G):
        self.phase, self.W, self.G, self.P = phase, W, G, int(W.shape[0])


def _scheduled_rates(beta, gamma, graph, T) -> _SirSchedule:
    """beta and / or gamma is a RateSchedule: every value checked as the constant it stands for and restated as the most
    general form -- per-edge weights (w[q] = beta[col[q]] for a number or per-node rates) and per-node gamma -- per joint
    phase.  Raises ValueError before the library is entered."""
    n, nnz = int(graph.n), int(graph.nnz)
    if int(T) < 1:
        raise ValueError(f"a scheduled call needs T >= 1 (got {T})")
    col = None

    def edge_table(v):
        nonlocal col
        if isinstance(v, EdgeRates):
            if (v.n, v.nnz) != (n, nnz):
                raise ValueError(f"EdgeRates of a graph with {v.n} nodes / {v.nnz} entries given for one with {n} / {nnz}")
            return v.w
        b = _node_rates("beta", v, n)
        if b is None:
            b = _node_rates("beta", np.full(n, float(v)), n)        # the scalar, through the same check
        if col is None:
            col = _host_csr(graph)[2]
        return b[col]

    def node_table(v):
        if isinstance(v, EdgeRates):
            raise ValueError("gamma: a recovery rate is a number or per-node rates, not EdgeRates")
        g = _node_rates("gamma", v, n)
        return _node_rates("gamma", np.full(n, float(v)), n) if g is None else g

    b_vals, g_vals = (s.values if isinstance(s, RateSchedule) else [s] for s in (beta, gamma))
    b_tabs, g_tabs = [edge_table(v) for v in b_vals], [node_table(v) for v in g_vals]
    rows = [s.phase_of_step(T) if isinstance(s, RateSchedule) else np.zeros(int(T), dtype=np.int32) for s in (beta, gamma)]
    phase, pairs = joint_phases(rows)
    W = np.ascontiguousarray(np.stack([b_tabs[pb] for pb, _ in pairs]).reshape(len(pairs), nnz), dtype=np.float64)
    G = np.ascontiguousarray(np.stack([g_tabs[pg] for _, pg in pairs]), dtype=np.float64)
    return _SirSchedule(phase, W, G)


def _resolved_rates(beta, gamma, graph, T=None):
    """(b, g) for one launch: an EdgeRates and gamma as given (checked), two float64 [n] host arrays when either rate is per
    node, else two numbers; a `_SirSchedule` and None when either is a `RateSchedule` (T is then the call's).  Raises
    ValueError before anything is allocated."""
    n = graph.n
    if isinstance(beta, RateSchedule) or isinstance(gamma, RateSchedule):
        return _scheduled_rates(beta, gamma, graph, T), None
    if isinstance(beta, EdgeRates):
        _edge_rate_args(beta, gamma, graph)
        return beta, gamma
    b, g = _node_rates("beta", beta, n), _node_rates("gamma", gamma, n)
    if b is not None or g is not None:
        b = _node_rates("beta", np.full(n, float(beta)), n) if b is None else b
        g = _node_rates("gamma", np.full(n, float(gamma)), n) if g is None else g
        return b, g
    return float(beta), float(gamma)


def _init_for(init: InitialState, n: int) -> InitialState:
    if init.n != n:
        raise ValueError(f"InitialState of {init.n} nodes given for a graph of {n}")
    return init


# (rate form 0 scalar / 1 per node / 2 per edge, per-trajectory output) -> the seed-list C entry, its workspace-size entry and
# which of the rate arguments (beta, beta_host, w_host, gamma, gamma_host) it takes, in its order
_SIR_ENTRIES = {
    (0, False): ("gnode_sir_mc_philox", "gnode_sir_workspace_bytes", (0, 3)),
    (1, False): ("gnode_sir_mc_philox_nodes", "gnode_sir_nodes_workspace_bytes", (1, 4)),
    (2, False): ("gnode_sir_mc_philox_edges", "gnode_sir_edges_workspace_bytes", (2, 3, 4)),
    (0, True): ("gnode_sir_mc_philox_traj", "gnode_sir_traj_workspace_bytes", (0, 3, 1, 4)),
    (1, True): ("gnode_sir_mc_philox_traj", "gnode_sir_traj_workspace_bytes", (0, 3, 1, 4)),
    (2, True): ("gnode_sir_mc_philox_traj_edges", "gnode_sir_edges_workspace_bytes", (2, 3, 4)),
}
_SIR_INIT_ENTRY = ("gnode_sir_mc_philox_init", "gnode_sir_init_workspace_bytes", (0, 1, 2, 3, 4))


def _sir_launch(graph: DeviceGraph, start, b, g, sims, T, rng_seed, sim_offset, ev, cv, counts, edge_scan, entry=None, extra=()):
    """One Monte-Carlo launch into ev (int16 [2, sims, n]), cv (int32 [sims, T, 3]) and counts (int32 [3, T, n], accumulated);
    each may be None, not all.  start: a seed list or an `InitialState`; b / g: as `_resolved_rates` returns them.  `entry`
    names a C entry that takes the scalar seed-list entry's arguments (then `extra` behind them) in its place."""
    lib = _lib.load()
    drawn, traj = isinstance(start, InitialState), ev is not None or cv is not None
    if isinstance(b, _SirSchedule):                                 # one entry for both starts and every output
        seeds = None if drawn else np.ascontiguousarray(list(start), dtype=np.int32)
        start_args = (None, 0, _lib.host_ptr(start.p)) if drawn else (_lib.host_ptr(seeds), int(seeds.shape[0]), None)
        dev = next(t for t in (counts, ev, cv) if t is not None).device
        ws = torch.empty(lib.gnode_sir_schedule_workspace_bytes(graph.handle, int(T), b.P), dtype=torch.uint8, device=dev)
        _lib.check(lib.gnode_sir_mc_philox_schedule(graph.handle, *start_args, _lib.host_ptr(b.phase), b.P, _lib.host_ptr(b.W), _lib.host_ptr(b.G),
                                                    int(sims), int(sim_offset), int(T), C.c_uint64(int(rng_seed) & (2**64 - 1)), _lib.ptr(ev),
                                                    _lib.ptr(cv), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(),
                                                    int(bool(edge_scan))))
        return
    if isinstance(b, EdgeRates):
        (w, gam, gam_host), _alive = _edge_rate_args(b, g, graph)
        form, rates = 2, (0.0, None, w, gam, gam_host)
    elif isinstance(b, np.ndarray):
        form, rates = 1, (0.0, _lib.host_ptr(b), None, 0.0, _lib.host_ptr(g))
    else:
        form, rates = 0, (float(b), None, None, float(g), None)
    name, ws_name, takes = _SIR_INIT_ENTRY if drawn else _SIR_ENTRIES[(form, traj)]
    if drawn:
        start_args = (_lib.host_ptr(start.p),)
    else:
        seeds = np.ascontiguousarray(list(start), dtype=np.int32)
        start_args = (_lib.host_ptr(seeds), int(seeds.shape[0]))
    scalar_entry = not drawn and form == 0 and not traj             # ... and its _scan / _counted siblings: no edge_scan argument
    if scalar_entry and edge_scan:
        name = "gnode_sir_mc_philox_scan"
    dev = next(t for t in (counts, ev, cv) if t is not None).device
    ws = torch.empty(getattr(lib, ws_name)(graph.handle, T), dtype=torch.uint8, device=dev)
    outputs = (_lib.ptr(ev), _lib.ptr(cv)) if drawn or traj else ()
    _lib.check(getattr(lib, entry or name)(graph.handle, *start_args, *(rates[i] for i in takes), int(sims), int(sim_offset), int(T),
                                           C.c_uint64(int(rng_seed) & (2**64 - 1)), *outputs, _lib.ptr(counts), _lib.ptr(ws), ws.numel(),
                                           _lib.stream_ptr(), *(() if scalar_entry else (int(bool(edge_scan)),)), *extra))


def sir_counts(graph: DeviceGraph, seed_set, beta, gamma, sims, T, rng_seed, sim_offset=0, device="cuda",
               counts: torch.Tensor | None = None, edge_scan: bool = False) -> torch.Tensor:
    """Production Monte-Carlo on the GPU: uint32 (stored as int32 tensor) counts [3, T, n].

    `counts` may be passed to accumulate several shards of the sims range into one array.  edge_scan=True runs the
    edge-parallel statement of the same model (`gnode_sir_mc_philox_scan`: identical counts, O(nnz) per step).

    beta and gamma are, independently, one number for the graph or per-node rates of length graph.n (numpy array, list,
    torch tensor): beta[v] is the probability that an infected neighbour infects the susceptible v in a step (indexed by
    the target, as x[:, 3] of the GN-ODE), gamma[u] that the infected u recovers.  Two numbers take the scalar entry as
    before; anything else goes through `gnode_sir_mc_philox_nodes` (same coins: constant arrays give the scalar counts),
    which synchronises the stream.  A wrong length, a NaN or a value outside [0, 1] raises ValueError.

    beta may also be an `EdgeRates` (from `edge_rates`): one transmission probability per directed CSR entry, source = row,
    target = column, through `gnode_sir_mc_philox_edges`; gamma stays a number or per-node rates.

    seed_set may be an `InitialState` (from `initial_state` / `InitialState.from_sets`): every trajectory then draws its
    start from the per-node (pS, pI, pR), through `gnode_sir_mc_philox_init`, with any of the rate forms above.  Row 0 of
    the counts is then ACCUMULATED like the other rows (how many trajectories start in S / I / R); a state that is one-hot
    I on a seed set and S elsewhere gives the seed-list call's rows t >= 1 exactly.  A wrong n raises ValueError.

    beta and / or gamma may be a `RateSchedule` (from `rate_schedule`): the rate then changes at given steps -- contacts cut
    to 30 % from day 10, weekends unlike weekdays.  beta's values are numbers, per-node arrays or `EdgeRates`, mixed freely;
    gamma's are numbers or per-node arrays; the two schedules need not change at the same steps.  Step t draws the coins it
    always drew and holds them against the thresholds of the values that govern step t (`gnode_sir_mc_philox_schedule`), so
    a schedule of one value returns the constant call's counts.  Every start, output, shard and edge_scan works as above."""
    if isinstance(seed_set, InitialState):
        _init_for(seed_set, graph.n)
    b, g = _resolved_rates(beta, gamma, graph, T)                   # (ValueError before the library is entered)
    if counts is None:
        counts = torch.zeros((3, T, graph.n), dtype=torch.int32, device=device)
    _sir_launch(graph, seed_set, b, g, sims, T, rng_seed, sim_offset, None, None, counts, edge_scan)
    return counts


class SirTrajectories(NamedTuple):
    """What `sir_trajectories` returns; a field is None where it was not requested."""
    t_inf: torch.Tensor | None      # int16 [sims, n]: step at which the node was infected (0: a seed), -1 never within T
    t_rec: torch.Tensor | None      # int16 [sims, n]: step at which it recovered, -1 never within T
    curves: torch.Tensor | None     # int32 [sims, T, 3]: (S_t, I_t, R_t) of each trajectory


def sir_trajectories(graph_or_G, seed_set, beta, gamma, sims, T, rng_seed=None, sim_offset=0, events=True, curves=True,
                     counts: torch.Tensor | None = None, edge_scan: bool = False, device="cuda") -> SirTrajectories:
    """The Monte-Carlo of `sir_counts`, trajectory by trajectory: `SirTrajectories(t_inf, t_rec, curves)` on the GPU.

    Each of the `sims` trajectories is described by two steps per node -- t_inf[s, v], when v was infected (0 for a seed),
    and t_rec[s, v], when it recovered; -1 = never within T; t_rec > t_inf wherever both are set -- and by its population
    totals curves[s, t] = (S_t, I_t, R_t), whose row 0 is the true initial state.  s counts inside the call: trajectory s
    draws the coins of sim_offset + s, so trajectories [a, b) of a large run are the call with sims = b - a, sim_offset = a
    (events take 4 * sims * n bytes: shard large runs).  `sir_state_at`, `sir_counts_from_events` and
    `sir_curves_from_events` read the events; the second returns what `sir_counts` of the same arguments returns.

    graph_or_G: a DeviceGraph or a networkx graph.  beta / gamma: as in `sir_counts` (an `EdgeRates` for beta included).  rng_seed=None draws the seed from
    torch's CPU generator, as `sir_torch` does.  events=False / curves=False leave that output out (None in the result);
    `counts` (int32 [3, T, n]) is accumulated into as by `sir_counts`.  edge_scan=True runs the edge-parallel kernel.
    seed_set may be an `InitialState`, as in `sir_counts`: a node that starts in I has t_inf = 0, one that starts in R has
    t_inf = 0 and t_rec = 0 (the one case of t_rec == t_inf), and curves row 0 is the trajectory's drawn state.
    Raises ValueError for bad rates, for T > 32767 with events, and when neither output is requested."""
    graph = _device_graph_for(graph_or_G) if hasattr(graph_or_G, "number_of_nodes") else graph_or_G
    n = graph.n
    if isinstance(seed_set, InitialState):
        _init_for(seed_set, n)
    b, g = _resolved_rates(beta, gamma, graph, T)                   # (ValueError before anything is allocated)
    if not events and not curves:
        raise ValueError("sir_trajectories: neither events nor curves requested")
    if events and T > 32767:
        raise ValueError(f"sir_trajectories: events hold int16 steps, T = {T} > 32767")
    if rng_seed is None:
        rng_seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())
    dev = counts.device if counts is not None else device
    ev = torch.empty((2, sims, n), dtype=torch.int16, device=dev) if events else None
    cv = torch.empty((sims, T, 3), dtype=torch.int32, device=dev) if curves else None
    if sims > 0:
        _sir_launch(graph, seed_set, b, g, sims, T, rng_seed, sim_offset, ev, cv, counts, edge_scan)
    return SirTrajectories(ev[0] if events else None, ev[1] if events else None, cv)


def sir_state_at(t_inf: torch.Tensor, t_rec: torch.Tensor, t: int) -> torch.Tensor:
    """int8 [sims, n]: 0 S, 1 I, 2 R at step t -- infected means 0 <= t_inf <= t, recovered 0 <= t_rec <= t."""
    inf = (t_inf >= 0) & (t_inf <= t)
    rec = (t_rec >= 0) & (t_rec <= t)
    return inf.to(torch.int8) + rec.to(torch.int8)


def _events_up_to(t_ev: torch.Tensor, T: int, dim: int) -> torch.Tensor:
    """int32 cumulative event counts: along the other dimension of the [sims, n] event steps, how many are in [0, t], for
    t = 0 .. T - 1 (dim = 0: [T, n], summed over trajectories; dim = 1: [sims, T], summed over nodes)."""
    idx = torch.where(t_ev < 0, T, t_ev.to(torch.int64))                       # "never" goes to a row that is dropped
    shape = (T + 1, t_ev.shape[1]) if dim == 0 else (t_ev.shape[0], T + 1)
    hist = torch.zeros(shape, dtype=torch.int32, device=t_ev.device)
    hist.scatter_add_(dim, idx, torch.ones_like(idx, dtype=torch.int32))
    return hist.narrow(dim, 0, T).cumsum(dim, dtype=torch.int32)


def sir_counts_from_events(t_inf: torch.Tensor, t_rec: torch.Tensor, T: int, accumulate_t0: bool = False) -> torch.Tensor:
    """int32 [3, T, n]: the counts `sir_counts` accumulates for these trajectories -- rows t >= 1 the number of
    trajectories in which the node is S / I / R at step t, row 0 the initial state ONCE (the reference's quirk).
    accumulate_t0=True counts row 0 like the other rows: what `sir_counts` of an `InitialState` returns."""
    sims = t_inf.shape[0]
    ci, cr = _events_up_to(t_inf, T, 0), _events_up_to(t_rec, T, 0)
    out = torch.stack([sims - ci, ci - cr, cr])
    if accumulate_t0:
        return out
    seeded = (t_inf == 0).any(dim=0).to(torch.int32)                           # every trajectory starts from the same seeds
    out[0, 0], out[1, 0], out[2, 0] = 1 - seeded, seeded, 0
    return out


def sir_curves_from_events(t_inf: torch.Tensor, t_rec: torch.Tensor, T: int) -> torch.Tensor:
    """int32 [sims, T, 3]: (S_t, I_t, R_t) of each trajectory, row 0 the true initial state."""
    n = t_inf.shape[1]
    ci, cr = _events_up_to(t_inf, T, 1), _events_up_to(t_rec, T, 1)
    return torch.stack([n - ci, ci - cr, cr], dim=2)


class SirOutbreakSizes(NamedTuple):
    """What `outbreak_sizes_mc` returns."""
    sums: torch.Tensor              # int64 [C, T, 3]: (S_t, I_t, R_t) summed over the trajectories of each candidate
    ever: torch.Tensor | None       # int32 [C, sims]: nodes ever infected in each trajectory; None unless per_trajectory
    sims: int                       # the trajectories per candidate of THIS call

    def sizes(self) -> torch.Tensor:
        """float64 [C, T, 3] = sums / sims: the table `gnode.dmp.outbreak_sizes` gives, from the Monte-Carlo; `gnode.dmp.infections`
        reads it unchanged.  (After accumulating shards into one `sums`, divide by the total yourself.)"""
        return self.sums.double() / float(self.sims)


class _HostGraph:
    """n, nnz and the host CSR of a graph argument, before any graph handle exists."""

    def __init__(self, graph):
        self.n, rp, ci = _host_csr(graph)
        self.rowptr, self.col, self.nnz = rp, ci, int(ci.shape[0])


def _whole(who, name, value, lowest):
    if isinstance(value, (bool, str)) or not isinstance(value, (int, float, np.integer, np.floating)) or value != int(value) or value < lowest:
        raise ValueError(f"{who}: {name} must be a whole number >= {lowest}, got {value!r}")
    return int(value)


_MC_ACTIONS = {"seed": 0, "immunise": 1}


def outbreak_sizes_mc(graph, beta, gamma, sims, maxTime, candidates=None, action="seed", start=None, shifts=None, rng_seed=None,
                      sim_offset=0, per_trajectory=False, edge_scan=False, device="cuda", sums: torch.Tensor | None = None) -> SirOutbreakSizes:
    """`gnode.dmp.outbreak_sizes` / `outbreak_sizes_schedule` by Monte-Carlo, every candidate in ONE launch: for each candidate
    node c, the compartment sizes over time of `sims` trajectories that start from `start` with c alone changed --
    action="seed": c starts infected; action="immunise": c starts removed.  Returns `SirOutbreakSizes(sums, ever, sims)`:
    sums int64 [C, maxTime, 3] on the GPU, sums[c, t] = (S_t, I_t, R_t) added over the trajectories (row 0 is the start after
    the change; exact integers, whatever the launch geometry); ever int32 [C, sims] when per_trajectory=True, the number of nodes
    of each trajectory that were ever infected (I starts count, R starts do not), else None.  `.sizes()` is sums / sims, the
    table DMP approximates; `gnode.dmp.infections` reads it.  DMP is exact on trees only: this is the ground truth to hold its
    ranking against on a graph with loops.

    Trajectory s of every candidate draws the coins of sim_offset + s: the candidates are compared on common random numbers,
    and a candidate's rows do not depend on the other candidates.  graph: a DeviceGraph, a networkx graph or a (rowptr, col)
    pair.  beta / gamma: everything `sir_trajectories` takes -- numbers, per-node arrays, `EdgeRates`, a `RateSchedule` of them.
    start: None (everybody susceptible), a seed list or an `InitialState`; "immunise" needs some infected mass in it.
    candidates: node ids (repeats allowed), every node by default; -1 means "no change".  shifts: None, or one whole number >= 0
    per candidate: step t of candidate c's run is governed by the schedules' step shifts[c] + t (they are read up to step
    max(shifts) + maxTime - 1), while the coins stay those of the run's own step t.  sums=: an int64 [C, maxTime, 3] tensor to
    ACCUMULATE into, for shards of the sims range (sim_offset).  edge_scan=True runs the edge-parallel kernel (same integers).
    Through `gnode_sir_mc_philox_sweep`, which synchronises the stream.  What is wrong raises ValueError before the library is
    loaded or a graph handle is made."""
    a = _McSweep("outbreak_sizes_mc", graph, beta, gamma, sims, maxTime, candidates, action, start, shifts, sim_offset)
    sums, ever = a.launch("gnode_sir_mc_philox_sweep", "gnode_sir_sweep_workspace_bytes", [("sums", sums, (a.C, a.T, 3))], rng_seed, edge_scan, device,
                          written=[(a.C, a.sims) if per_trajectory else None])
    return SirOutbreakSizes(sums, ever, a.sims)


def _accumulator(who, name, t, shape):
    """ValueError unless t is None or a contiguous int64 tensor of `shape` (an output to accumulate shards into)"""
    if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous()):
        raise ValueError(f"{who}: {name} must be a contiguous int64 tensor of shape {tuple(shape)}")


def _mc_bins(who, bins):
    """The bins of a Monte-Carlo scorer's histogram: a whole number in 1 .. 4096."""
    bins = _whole(who, "bins", bins, 1)
    if bins > 4096:
        raise ValueError(f"{who}: bins = {bins} exceeds 4096")
    return bins


def _mc_groups(evidence, group):
    """(o0, og, evidence arguments, sizes for the workspace query) per launch of a candidate sweep.  `evidence` None: one
    launch without evidence, its outputs whole (o0 None).  Snapshot rows (int8 [O, n]) or evidence sets (_timed_records): the
    rows or sets o0 .. o0 + og - 1, `group` at a time -- the rows as they are, the sets' records as four int32 arrays, `which`
    naming each record's set within the group."""
    if evidence is None:
        yield None, None, (), ()
        return
    for o0 in range(0, len(evidence), group):
        part = evidence[o0:o0 + group]
        og = len(part)
        if isinstance(part, np.ndarray):
            yield o0, og, (_lib.host_ptr(part), og), (og,)
            continue
        which = np.concatenate([np.full(len(s[0]), i, dtype=np.int32) for i, s in enumerate(part)])
        node, off, kind = (np.ascontiguousarray(np.concatenate([s[j] for s in part])) for j in range(3))
        yield o0, og, (*(_lib.host_ptr(x) for x in (which, node, off, kind)), len(which), og), (og, len(which))


def _mc_horizons(who, now, horizons, T):
    """(now, the horizons int64 [H], their int32 copy) of a posterior call: now in [0, T), 1 to SIR_POST_MAXH ascending whole
    numbers >= 0 (one number is one horizon) with now + h <= T - 1; ValueError otherwise."""
    now = _whole(who, "now", now, 0)
    if now >= T:
        raise ValueError(f"{who}: now = {now} is not in [0, maxTime = {T})")
    if isinstance(horizons, (int, float, np.integer, np.floating)) and not isinstance(horizons, bool):
        horizons = (horizons,)
    hz = _whole_numbers(who, "horizons", horizons)
    if hz.ndim != 1 or not 1 <= hz.size <= SIR_POST_MAXH:
        raise ValueError(f"{who}: 1 to {SIR_POST_MAXH} horizons, got {hz.size}")
    if hz[0] < 0 or (np.diff(hz) <= 0).any():
        j = 0 if hz[0] < 0 else int(np.flatnonzero(np.diff(hz) <= 0)[0]) + 1
        raise ValueError(f"{who}: horizons[{j}] = {int(hz[j])}: horizons are whole numbers >= 0 in ascending order")
    if now + int(hz[-1]) > T - 1:
        j = int(np.flatnonzero(now + hz > T - 1)[0])
        raise ValueError(f"{who}: horizons[{j}] = {int(hz[j])}: now + horizon = {now + int(hz[j])} is past the last step maxTime - 1 = {T - 1}")
    return now, hz, np.ascontiguousarray(hz, dtype=np.int32)


class _McSweep:
    """The arguments `outbreak_sizes_mc`, `source_scores_mc`, `source_scores_timed_mc`, `posterior_states_mc` and
    `posterior_strata_mc` share, checked on the host (ValueError) before the library is loaded or a graph handle is made: the
    graph, maxTime / sims / sim_offset, the action, the start, the candidates, the shifts and the rates as one schedule over
    max(shifts) + maxTime calendar steps.  `launch` is then the one way into the library for all five."""

    def __init__(self, who, graph, beta, gamma, sims, maxTime, candidates, action, start, shifts, sim_offset):
        self.who, self.graph, self.made = who, graph, hasattr(graph, "handle")      # a DeviceGraph: it carries its host CSR
        self.host = host = graph if self.made else _HostGraph(graph)
        self.n = n = int(host.n)
        self.T, self.sims, self.sim_offset = _whole(who, "maxTime", maxTime, 1), _whole(who, "sims", sims, 0), _whole(who, "sim_offset", sim_offset, 0)
        T = self.T
        if self.sim_offset + self.sims > 0xFFFFFFFF:
            raise ValueError(f"{who}: sim_offset + sims = {self.sim_offset + self.sims} exceeds 2^32 - 1 trajectories")
        if action not in _MC_ACTIONS:
            raise ValueError(f"{who}: action must be one of {sorted(_MC_ACTIONS)}, got {action!r}")
        self.action = _MC_ACTIONS[action]
        if isinstance(start, InitialState):
            self.base = _init_for(start, n)
        else:
            self.base = InitialState.from_sets(n, [] if start is None else _whole_numbers(who, "start", start))    # (a seed outside the graph: ValueError)
        if action == "immunise" and not (self.base.p[:, 1] > 0.0).any():
            raise ValueError(f"{who}: nothing to immunise against: the start holds no infected mass")
        cand = np.arange(n, dtype=np.int64) if candidates is None else _whole_numbers(who, "candidates", candidates)
        if cand.size < 1:
            raise ValueError(f"{who}: need at least one candidate")
        if cand.min() < -1 or cand.max() >= n:
            raise ValueError(f"{who}: candidate {int(cand[(cand < -1) | (cand >= n)][0])} is not in [-1, {n})")
        self.C = C_ = int(cand.size)
        if shifts is None:
            sh = np.zeros(C_, dtype=np.int64)
        else:
            sh = _whole_numbers(who, "shifts", shifts)
            if sh.shape[0] != C_:
                raise ValueError(f"{who}: {C_} candidates need {C_} shifts, got {sh.shape[0]}")
            if sh.min() < 0:
                raise ValueError(f"{who}: shift {int(sh.min())} is negative: a run starts at calendar step 0 or later")
        self.L = int(sh.max()) + T
        if self.L > 2**31 - 1:
            raise ValueError(f"{who}: max(shifts) + maxTime = {self.L} does not fit an int32")
        self.sched = _scheduled_rates(beta, gamma, host, self.L)    # constants become one phase
        self.cand32, self.sh32 = np.ascontiguousarray(cand, dtype=np.int32), np.ascontiguousarray(sh, dtype=np.int32)

    def enter(self, rng_seed):
        """(graph handle's owner, library, rng seed as a uint64): everything was in order"""
        if rng_seed is None:
            rng_seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())
        graph, host = self.graph, self.host
        g = graph if self.made else _device_graph_for(graph) if hasattr(graph, "number_of_nodes") else DeviceGraph(host.rowptr, host.col)
        return g, _lib.load(), int(rng_seed) & (2**64 - 1)

    def sweep_args(self):
        """the entries' arguments from init_host to gamma_host"""
        s = self.sched
        return (_lib.host_ptr(self.base.p), _lib.host_ptr(self.cand32), _lib.host_ptr(self.sh32), self.C, self.action, _lib.host_ptr(s.phase), s.P,
                self.L, _lib.host_ptr(s.W), _lib.host_ptr(s.G))

    def launch(self, entry, query, outputs, rng_seed, edge_scan, device, evidence=None, group=None, scalars=(), query_scalars=(), cells=None, written=()):
        """The last checks, then the launches of `entry`; returns the output tensors, `outputs` and then `written`, in order.
        outputs: (name, the caller's tensor or None, shape) of each int64 accumulator, by _accumulator; two given ones on different
        devices are refused, the first given one names the device (else `device`), a missing one is allocated as zeros.
        written: the shape, or None for an output not wanted, of each int32 output that is written and not accumulated.
        evidence / group: see _mc_groups; a grouped launch gets rows [o0, o0 + og) of every accumulator (contiguous: o is their
        slowest axis), and cells = (noun, advice) refuses a first accumulator of 2^31 cells or more per launch.  Per launch the
        workspace is sized by `query`(handle, T, P, L, C, the group's sizes, *query_scalars) and the entry takes (handle,
        sweep_args, the group's evidence, *scalars, sims, sim_offset, T, seed, the outputs, workspace, its bytes, stream,
        edge_scan).  sims == 0: the graph handle is made, nothing is queried or launched."""
        who = self.who
        if cells is not None:
            factors = (min(len(evidence), group), *outputs[0][2][1:])
            if math.prod(factors) >= 2**31:
                raise ValueError(f"{who}: {' x '.join(str(f) for f in factors)} {cells[0]} cells per launch reach 2^31: {cells[1]}")
        for name, t, shape in outputs:
            _accumulator(who, name, t, shape)
        given = [(name, t) for name, t, _ in outputs if t is not None]
        for (first, t), (second, u) in zip(given, given[1:]):
            if t.device != u.device:
                raise ValueError(f"{who}: {first} is on {t.device} and {second} on {u.device}")
        g, lib, seed = self.enter(rng_seed)
        dev = given[0][1].device if given else device
        outs = [torch.zeros(shape, dtype=torch.int64, device=dev) if t is None else t for _, t, shape in outputs]
        more = [None if shape is None else torch.empty(shape, dtype=torch.int32, device=dev) for shape in written]
        for o0, og, ev_args, ev_sizes in _mc_groups(evidence, group) if self.sims > 0 else ():
            ws = torch.empty(getattr(lib, query)(g.handle, self.T, self.sched.P, self.L, self.C, *ev_sizes, *query_scalars), dtype=torch.uint8, device=dev)
            part = outs if o0 is None else [t[o0:o0 + og] for t in outs]
            _lib.check(getattr(lib, entry)(g.handle, *self.sweep_args(), *ev_args, *scalars, self.sims, self.sim_offset, self.T, C.c_uint64(seed),
                                           *(_lib.ptr(t) for t in part + more), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(), int(bool(edge_scan))))
        return (*outs, *more)


SIR_SCORE_MAXO = 16                                                 # GN_SIR_SCORE_MAXO of the library as built: snapshots per launch
_MC_MEASURES = {"jaccard": 0, "match": 1}


class SirSourceScores(NamedTuple):
    """What `source_scores_mc` returns."""
    hist: torch.Tensor              # int64 [O, C, T, bins + 1]: trajectories of candidate c whose step t fell into bin k of snapshot o
    sims: int                       # the trajectories per candidate of THIS call
    bins: int
    squeezed: bool                  # `obs` was one row: exact() and scores() drop the snapshot axis

    def _table(self, x):
        return x[0] if self.squeezed else x

    def exact(self) -> torch.Tensor:
        """float64 [O, C, T] ([C, T] for one snapshot): hist[..., bins] / sims, the share of the trajectories that agree with the
        snapshot on every observed node -- an unbiased estimate of the true likelihood (the kernel of width -> 0)."""
        return self._table(self.hist[..., self.bins].double() / float(self.sims))

    def scores(self, width=0.25, floor=1e-30) -> torch.Tensor:
        """float64 [O, C, T] ([C, T] for one snapshot): log max(floor, sum_k hist[..., k] exp(-(1 - k / bins)^2 / width^2) / sims),
        the soft-margin estimator's log-likelihood of (source, onset) -- a bin is taken at its lower edge, the top bin is phi = 1
        exactly.  `gnode.dmp.rank_sources` and `source_rank_of` read it unchanged.  (After accumulating shards into one `hist`,
        build the result with the total sims.)"""
        if not width > 0.0:
            raise ValueError(f"SirSourceScores.scores: width must be > 0, got {width!r}")
        k = torch.arange(self.bins + 1, dtype=torch.float64, device=self.hist.device)
        wgt = torch.exp(-(1.0 - k / float(self.bins)) ** 2 / float(width) ** 2)
        return self._table(torch.log(torch.clamp((self.hist.double() * wgt).sum(-1) / float(self.sims), min=float(floor))))


def source_scores_mc(graph, obs, beta, gamma, sims, maxTime, candidates=None, start=None, shifts=None, measure="jaccard", bins=64, rng_seed=None,
                     sim_offset=0, edge_scan=False, device="cuda", hist: torch.Tensor | None = None) -> SirSourceScores:
    """`gnode.dmp.source_scores` by Monte-Carlo, the soft-margin estimator of Antulov-Fantulin et al. (PRL 2015): for each
    candidate source c, `sims` trajectories start from `start` with c infected -- the trajectories of `outbreak_sizes_mc`,
    action "seed" -- and the state of each at every step t = 0 .. maxTime - 1 is compared with the observed snapshot(s).  All
    candidates and up to 16 snapshots share ONE launch; nothing per trajectory reaches memory.  Returns
    `SirSourceScores(hist, sims, bins, squeezed)`: hist int64 [O, C, maxTime, bins + 1] on the GPU, the number of trajectories
    whose similarity with snapshot o fell into bin k -- exact integers, whatever the launch geometry; `.exact()` is the
    exact-match frequency, `.scores(width)` the log of the Gaussian kernel's average, which `gnode.dmp.rank_sources` ranks.  DMP's
    source likelihood is a product of marginals of an approximation that is exact on trees only: this is what to hold it against
    on a graph with loops.

    obs: int8 codes [n] or [O, n] -- -1 not observed, 0 / 1 / 2 = S / I / R, as `source_scores` takes them and `sir_state_at`
    gives them -- numpy or a torch tensor on any device (copied to the host: O * n bytes); every snapshot observes some node.
    More than 16 snapshots run in groups of 16 on one graph handle.  measure: "jaccard" -- |A & B| / |A | B| of A = the nodes
    observed infected or recovered and B = the observed nodes that have left S -- or "match", the share of the observed nodes
    whose state equals the code.  bins: 1 .. 4096; bin k = floor(phi * bins) in integers, so the top bin is complete agreement.
    candidates, -1, start, shifts, beta / gamma (a `RateSchedule` included), sim_offset, edge_scan: as in `outbreak_sizes_mc`.
    hist=: an int64 [O, C, maxTime, bins + 1] tensor to ACCUMULATE into, for shards of the sims range.  Through
    `gnode_sir_mc_philox_sweep_scores`, which synchronises the stream.  What is wrong raises ValueError before the library is
    loaded or a graph handle is made."""
    who = "source_scores_mc"
    a = _McSweep(who, graph, beta, gamma, sims, maxTime, candidates, "seed", start, shifts, sim_offset)
    if measure not in _MC_MEASURES:
        raise ValueError(f"{who}: measure must be one of {sorted(_MC_MEASURES)}, got {measure!r}")
    bins = _mc_bins(who, bins)
    if isinstance(obs, torch.Tensor):
        obs = obs.detach().cpu().numpy()
    ob = np.asarray(obs)
    if ob.dtype.kind not in "iu" or ob.ndim not in (1, 2) or ob.shape[-1] != a.n or ob.shape[0] < 1:
        raise ValueError(f"{who}: obs must hold whole-number codes of shape [{a.n}] or [O, {a.n}], got {ob.dtype} {tuple(ob.shape)}")
    squeezed = ob.ndim == 1
    ob = np.atleast_2d(ob)
    if ob.min() < -1 or ob.max() > 2:
        o, v = (int(i[0]) for i in np.nonzero((ob < -1) | (ob > 2)))
        raise ValueError(f"{who}: obs[{o}][{v}] = {int(ob[o, v])} is not a code in [-1, 2]")
    blind = np.flatnonzero((ob >= 0).sum(1) == 0)
    if blind.size:
        raise ValueError(f"{who}: snapshot {int(blind[0])} observes no node")
    ob = np.ascontiguousarray(ob, dtype=np.int8)
    hist, = a.launch("gnode_sir_mc_philox_sweep_scores", "gnode_sir_sweep_scores_workspace_bytes", [("hist", hist, (int(ob.shape[0]), a.C, a.T, bins + 1))],
                     rng_seed, edge_scan, device, evidence=ob, group=SIR_SCORE_MAXO, scalars=(_MC_MEASURES[measure], bins),
                     cells=("histogram", "fewer bins or candidates"))
    return SirSourceScores(hist, a.sims, bins, squeezed)


SIR_TIMED_CELLS = 2048                                              # GN_SIR_TIMED_CELLS of the library as built: sets x maxTime per launch


def _timed_records(who, observations, n):
    """(squeezed, [(nodes, offsets, kinds) int32 [R_o]] per evidence set) of what `gnode.dmp.timed_observations` returns, or a
    sequence of them, taken by the attributes `.rows`, `.row_offsets` and `.n`; a record is every rows[r, v] >= 0, at offset
    row_offsets[r], in the order of the rows and then of the nodes.  ValueError for anything else."""
    squeezed = hasattr(observations, "rows")
    try:
        sets = [observations] if squeezed else list(observations)
    except TypeError:
        raise ValueError(f"{who}: observations must be what timed_observations returns, or a sequence of them, got {type(observations).__name__}") from None
    if not sets:
        raise ValueError(f"{who}: need at least one evidence set")
    out = []
    for o, s in enumerate(sets):
        if not all(hasattr(s, name) for name in ("rows", "row_offsets", "n")):
            raise ValueError(f"{who}: evidence set {o} has no .rows, .row_offsets and .n: not what timed_observations returns ({type(s).__name__})")
        rows, off = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (s.rows, s.row_offsets))
        if rows.dtype.kind not in "iu" or rows.ndim != 2 or rows.shape[1] != n or s.n != n:
            raise ValueError(f"{who}: evidence set {o}: rows must hold whole-number codes of shape [R, {n}], got {rows.dtype} {tuple(rows.shape)} (n = {s.n!r})")
        if off.dtype.kind not in "iu" or off.shape != (rows.shape[0],):
            raise ValueError(f"{who}: evidence set {o}: {rows.shape[0]} rows need {rows.shape[0]} whole-number row_offsets, got {off.dtype} {tuple(off.shape)}")
        if rows.size and (rows.min() < -1 or rows.max() > 4):
            r, v = (int(i[0]) for i in np.nonzero((rows < -1) | (rows > 4)))
            raise ValueError(f"{who}: evidence set {o}: rows[{r}][{v}] = {int(rows[r, v])} is not a kind in [-1, 4]")
        if off.size and off.max() > 0:
            raise ValueError(f"{who}: evidence set {o}: offset {int(off.max())} is after now: offsets are <= 0")
        r, v = np.nonzero(rows >= 0)
        if r.size < 1:
            raise ValueError(f"{who}: evidence set {o} holds no record")
        back = np.maximum(off.astype(np.int64)[r], -(2**31 - 1))   # (beyond maxTime steps back every offset reads "before the outbreak")
        out.append((v.astype(np.int32), back.astype(np.int32), rows[r, v].astype(np.int32)))
    return squeezed, out


def source_scores_timed_mc(graph, observations, beta, gamma, sims, maxTime, candidates=None, start=None, shifts=None, bins=None, rng_seed=None,
                           sim_offset=0, edge_scan=False, device="cuda", hist: torch.Tensor | None = None) -> SirSourceScores:
    """`gnode.dmp.source_scores_timed` by Monte-Carlo: which node started the outbreak, from records taken at DIFFERENT times --
    onsets at a few sensors, recovery dates, tests on different days, two records for one person?  For each candidate source c,
    `sims` trajectories start from `start` with c infected -- the trajectories of `source_scores_mc` -- and each is compared, for
    every possible age t = 0 .. maxTime - 1 of the outbreak, with ALL records of an evidence set jointly: a record (node v,
    offset d <= 0, kind) is read at the trajectory's step t + d -- kind 0 / 1 / 2: v was S / I / R then; 3: v became infected at
    that step; 4: v recovered at that step; before the outbreak (t + d < 0) everybody is susceptible.  Returns
    `SirSourceScores(hist, sims, bins, squeezed)`: hist int64 [O, C, maxTime, bins + 1] on the GPU, the number of trajectories of
    candidate c that at age t agree with agree * bins // records of set o's records in bin k -- exact integers, whatever the
    launch geometry.  `.exact()` = hist[..., bins] / sims is an unbiased estimate of the JOINT likelihood P(all records | source
    c, age t), which DMP's timed score approximates twice over: by marginals that are exact on trees only, and by treating the
    records of one cascade as independent.  `.scores(width)`, `gnode.dmp.rank_sources` and `source_rank_of` work as for
    `source_scores_mc`.

    observations: what `gnode.dmp.timed_observations` returns (taken by its attributes `.rows` int8 [R, n], `.row_offsets` and
    `.n`), or a sequence of them for O evidence sets; one object gives [C, maxTime] tables.  A node may have several records.
    bins: 1 .. 4096; by default the largest record count of any set, so that this set is not binned at all (k = the number of
    matched records).  All candidates and up to min(16, 2048 // maxTime) sets share ONE launch -- the kernels keep sets x maxTime
    counters on chip -- and more sets run in groups on one graph handle; maxTime above 2048 is refused.  candidates, -1, start,
    shifts, beta / gamma (a `RateSchedule` included), sim_offset, edge_scan, hist=: as in `source_scores_mc`.  Through
    `gnode_sir_mc_philox_sweep_timed`, which synchronises the stream.  What is wrong raises ValueError before the library is
    loaded or a graph handle is made."""
    who = "source_scores_timed_mc"
    a = _McSweep(who, graph, beta, gamma, sims, maxTime, candidates, "seed", start, shifts, sim_offset)
    T = a.T
    if T > SIR_TIMED_CELLS:
        raise ValueError(f"{who}: maxTime = {T} exceeds the {SIR_TIMED_CELLS} steps one evidence set can be tallied over")
    squeezed, sets = _timed_records(who, observations, a.n)
    most = max(len(s[0]) for s in sets)
    if bins is None:
        if most > 4096:
            raise ValueError(f"{who}: an evidence set holds {most} records, more than 4096 bins: give bins")
        bins = most
    bins = _mc_bins(who, bins)
    hist, = a.launch("gnode_sir_mc_philox_sweep_timed", "gnode_sir_sweep_timed_workspace_bytes", [("hist", hist, (len(sets), a.C, T, bins + 1))],
                     rng_seed, edge_scan, device, evidence=sets, group=min(SIR_SCORE_MAXO, SIR_TIMED_CELLS // T), scalars=(bins,),
                     cells=("histogram", "fewer bins or candidates"))
    return SirSourceScores(hist, a.sims, bins, squeezed)


SIR_POST_MAXH = 32                                                  # GN_SIR_POST_MAXH of the library as built: horizons per launch


class SirPosterior(NamedTuple):
    """What `posterior_states_mc` returns."""
    counts: torch.Tensor            # int64 [O, H, 2, n]: accepted trajectories of all candidates with node v in I (plane 0) / R (plane 1) at now + h
    accepted: torch.Tensor          # int64 [O, C]: the accepted trajectories per evidence set and candidate
    sims: int                       # the trajectories per candidate of THIS call
    now: int
    horizons: tuple
    squeezed: bool                  # `observations` was one object: the methods drop the evidence-set axis

    def _table(self, x):
        return x[0] if self.squeezed else x

    def accepted_total(self) -> torch.Tensor:
        """int64 [O] (a scalar tensor for one evidence object): the accepted trajectories of all candidates"""
        return self._table(self.accepted.sum(-1))

    def source(self) -> torch.Tensor:
        """float64 [O, C] ([C]): accepted / accepted.sum(), the posterior over the candidates under a uniform prior (a repeated
        candidate carries its multiplicity); NaN where nothing was accepted"""
        a = self.accepted.double()
        return self._table(a / a.sum(-1, keepdim=True))

    def marginals(self) -> torch.Tensor:
        """float64 [O, H, n, 3] ([H, n, 3]): P(v is S, I, R at now + h | evidence) = (total - I - R, I, R) / total over the accepted
        trajectories, total = accepted.sum(); NaN where nothing was accepted"""
        tot = self.accepted.sum(-1)[:, None, None]
        i, r = self.counts[:, :, 0], self.counts[:, :, 1]
        return self._table(torch.stack([tot - i - r, i, r], dim=-1).double() / tot[..., None].double())


def posterior_states_mc(graph, observations, beta, gamma, sims, maxTime, now, horizons=(0,), candidates=None, start=None, shifts=None, rng_seed=None,
                        sim_offset=0, edge_scan=False, device="cuda", counts: torch.Tensor | None = None,
                        accepted: torch.Tensor | None = None) -> SirPosterior:
    """Nowcast and forecast from timed evidence by rejection sampling: given the records `source_scores_timed_mc` scores and the
    age `now` of the outbreak, who is infected now that nobody has tested, and who will be in h steps?  For each candidate source
    c, `sims` trajectories start from `start` with c infected -- the trajectories of `source_scores_timed_mc` -- and a trajectory
    is ACCEPTED for an evidence set when it matches EVERY record of the set at age `now` (a record (node v, offset d <= 0, kind)
    is read at step now + d, by that function's rule).  Returns `SirPosterior(counts, accepted, sims, now, horizons, squeezed)`:
    accepted int64 [O, C] on the GPU, the accepted trajectories per set and candidate; counts int64 [O, H, 2, n], over the
    accepted trajectories of ALL candidates those in which node v is infected (plane 0) or removed (plane 1) at step now +
    horizons[j] -- exact integers, whatever the launch geometry.  A trajectory that ended early keeps its final state.  Under a
    uniform prior over the candidates `.marginals()` = (S, I, R) / accepted.sum() is the posterior marginal of every node and
    `.source()` the posterior over the sources; repeats in `candidates` weigh the prior by their multiplicity, and a prior over
    starts that is not a single source goes through start=InitialState with candidates=[-1].  DMP cannot answer this: its
    marginals are unconditional.

    accepted[o, c] == source_scores_timed_mc(...).hist[o, c, now, bins] for the same seed; with an evidence set that is always
    matched (one kind-0 record further back than maxTime) accepted == sims everywhere and counts[o, j].sum(-1) is
    `outbreak_sizes_mc`'s sums[:, now + horizons[j], 1:3] summed over the candidates.

    observations: as in `source_scores_timed_mc`; one object drops the evidence-set axis in the methods.  now: a whole number in
    [0, maxTime).  horizons: 1 to 32 ascending whole numbers >= 0 with now + h <= maxTime - 1.  All candidates and up to 16 sets
    share ONE launch at any maxTime, more sets run in groups of 16 on one graph handle; a trajectory that no set of its group
    accepts ends at step `now`, and none runs past now + max(horizons).  candidates, -1, start, shifts, beta / gamma (a
    `RateSchedule` included), sim_offset, edge_scan: as in `outbreak_sizes_mc`.  counts=, accepted=: int64 tensors of the output
    shapes to ACCUMULATE into, for shards of the sims range.  Through `gnode_sir_mc_philox_sweep_posterior`, which synchronises
    the stream.  What is wrong raises ValueError before the library is loaded or a graph handle is made."""
    who = "posterior_states_mc"
    a = _McSweep(who, graph, beta, gamma, sims, maxTime, candidates, "seed", start, shifts, sim_offset)
    now, hz, hz32 = _mc_horizons(who, now, horizons, a.T)
    squeezed, sets = _timed_records(who, observations, a.n)
    O, H = len(sets), int(hz.size)
    counts, accepted = a.launch("gnode_sir_mc_philox_sweep_posterior", "gnode_sir_sweep_posterior_workspace_bytes",
                                [("counts", counts, (O, H, 2, a.n)), ("accepted", accepted, (O, a.C))], rng_seed, edge_scan, device,
                                evidence=sets, group=SIR_SCORE_MAXO, scalars=(now, _lib.host_ptr(hz32), H), query_scalars=(H,),
                                cells=("count", "fewer horizons"))
    return SirPosterior(counts, accepted, a.sims, now, tuple(int(h) for h in hz), squeezed)


SIR_POST_MAXD = 8                                                   # GN_SIR_POST_MAXD of the library as built: strata per launch


class SirPosteriorStrata(NamedTuple):
    """What `posterior_strata_mc` returns: the accepted trajectories kept apart by the number d of records they miss.  The
    methods weigh stratum d by w_d -- `error=e`: w_d = (e / (1 - e))^d, the posterior when EACH record independently disagrees
    with the truth with probability e (a missed test, a date remembered wrongly), whatever it reads instead; a particular wrong
    reading among several is the caller's to fold into `weights=`, a length-D sequence (flat: "at most M records are wrong").
    Exactly one of the two is given.  Where `.complete()` is false the strata beyond `mismatches` were dropped at step `now`,
    and the weighted posterior is that of the noisy records truncated there."""
    counts: torch.Tensor            # int64 [O, D, H, 2, n]: accepted trajectories of all candidates in stratum d with node v in I (plane 0) / R (plane 1) at now + h
    accepted: torch.Tensor          # int64 [O, C, D]: the accepted trajectories per evidence set, candidate and stratum
    sims: int                       # the trajectories per candidate of THIS call
    now: int
    horizons: tuple
    records: tuple                  # the record count of each evidence set
    squeezed: bool                  # `observations` was one object: the methods drop the evidence-set axis

    def _table(self, x):
        return x[0] if self.squeezed else x

    @property
    def mismatches(self) -> int:
        return int(self.accepted.shape[-1]) - 1

    def weights(self, error) -> torch.Tensor:
        """float64 [D]: (error / (1 - error)) ** d for 0 <= error < 1; error 0 gives (1, 0, ...), the exact-match posterior"""
        if isinstance(error, bool) or not isinstance(error, (int, float, np.integer, np.floating)) or not 0.0 <= float(error) < 1.0:
            raise ValueError(f"SirPosteriorStrata: error must be a number in [0, 1), got {error!r}")
        d = torch.arange(self.mismatches + 1, dtype=torch.float64, device=self.accepted.device)
        return torch.full_like(d, float(error) / (1.0 - float(error))) ** d          # (0 ** 0 is 1)

    def _w(self, who, error, weights):
        if (error is None) == (weights is None):
            raise ValueError(f"SirPosteriorStrata.{who}: give exactly one of error= and weights=")
        if weights is None:
            return self.weights(error)
        D = self.mismatches + 1
        try:
            w = np.asarray(weights, dtype=np.float64)
        except (TypeError, ValueError):
            w = None
        if w is None or w.shape != (D,) or not np.isfinite(w).all() or (w < 0).any() or not (w > 0).any():
            raise ValueError(f"SirPosteriorStrata.{who}: weights must be {D} finite numbers >= 0, not all zero, got {weights!r}")
        return torch.as_tensor(w, device=self.accepted.device)

    def by_stratum(self) -> torch.Tensor:
        """int64 [O, D] ([D]): the accepted trajectories of all candidates per stratum"""
        return self._table(self.accepted.sum(1))

    def source(self, error=None, weights=None) -> torch.Tensor:
        """float64 [O, C] ([C]): sum_d w_d accepted[o, c, d] over its sum over c, the posterior over the candidates under a
        uniform prior; NaN where nothing was accepted"""
        a = (self.accepted.double() * self._w("source", error, weights)).sum(-1)
        return self._table(a / a.sum(-1, keepdim=True))

    def marginals(self, error=None, weights=None) -> torch.Tensor:
        """float64 [O, H, n, 3] ([H, n, 3]): P(v is S, I, R at now + h | evidence) from the weighted counts over the weighted
        total; NaN where that total is 0"""
        w = self._w("marginals", error, weights)
        tot = (self.accepted.sum(1).double() * w).sum(-1)[:, None, None]
        c = (self.counts.double() * w[:, None, None, None]).sum(1)
        i, r = c[:, :, 0], c[:, :, 1]
        return self._table(torch.stack([tot - i - r, i, r], dim=-1) / tot[..., None])

    def ess(self, error=None, weights=None) -> torch.Tensor:
        """float64 [O] (a scalar tensor): the effective sample size (sum_d w_d A_d)^2 / sum_d w_d^2 A_d, A = `.by_stratum()`;
        NaN where nothing was accepted"""
        w = self._w("ess", error, weights)
        A = self.accepted.sum(1).double()
        return self._table((A * w).sum(-1) ** 2 / (A * w * w).sum(-1))

    def complete(self) -> torch.Tensor:
        """bool [O] (a scalar tensor): records[o] <= mismatches -- no stratum is cut off, every trajectory is accepted, and the
        weighted posterior is the noisy-record posterior exactly"""
        return self._table(torch.tensor([r <= self.mismatches for r in self.records], dtype=torch.bool))

    def exact(self) -> SirPosterior:
        """stratum 0 as `posterior_states_mc` returns it (views of the two tensors)"""
        return SirPosterior(self.counts[:, 0], self.accepted[:, :, 0], self.sims, self.now, self.horizons, self.squeezed)


def posterior_strata_mc(graph, observations, beta, gamma, sims, maxTime, now, horizons=(0,), mismatches=1, candidates=None, start=None,
                        shifts=None, rng_seed=None, sim_offset=0, edge_scan=False, device="cuda", counts: torch.Tensor | None = None,
                        accepted: torch.Tensor | None = None) -> SirPosteriorStrata:
    """`posterior_states_mc` from evidence that may be wrong: the same trajectories, records, `now` and horizons, but a
    trajectory that misses d of an evidence set's records is kept in STRATUM d as long as d <= `mismatches`, instead of being
    dropped at the first miss.  Returns `SirPosteriorStrata(counts, accepted, sims, now, horizons, records, squeezed)`: accepted
    int64 [O, C, D] on the GPU, D = mismatches + 1, the trajectories per set, candidate and stratum; counts int64 [O, D, H, 2, n],
    over the accepted trajectories of ALL candidates in stratum d those in which node v is infected (plane 0) or removed (plane
    1) at step now + horizons[j] -- exact integers, whatever the launch geometry.  Its methods turn the strata into posteriors:
    `.marginals(error=e)`, `.source(error=e)` and `.ess(error=e)` weigh stratum d by (e / (1 - e))^d, the posterior when each
    record INDEPENDENTLY disagrees with the truth with probability e -- for any e, chosen after the launch; `weights=` takes the
    strata's weights as given (flat: at most `mismatches` records are wrong; a particular wrong reading among several is the
    caller's to fold in there).  For a set with more records than `mismatches` (`.complete()` is false) the strata beyond
    `mismatches` are dropped, and the weighted posterior leaves out what they would add: the exact-match posterior's few
    accepted trajectories (an acceptance of one in a million for 18 records is usual) become the many that miss one or two.

    Stratum 0 is `posterior_states_mc`'s output for the same seed (`.exact()`), a smaller `mismatches` gives the first strata of
    a larger one, and accepted[o, c, d] == source_scores_timed_mc(set o).hist[c, now, R_o - d] with that function's default bins.

    mismatches: a whole number in [0, 7].  Everything else as in `posterior_states_mc`: all candidates and up to 16 sets share
    ONE launch, more sets run in groups of 16 on one graph handle; a trajectory that no set of its group accepts ends at step
    `now`, and none runs past now + max(horizons).  counts=, accepted=: int64 tensors of the output shapes to ACCUMULATE into,
    for shards of the sims range.  Through `gnode_sir_mc_philox_sweep_posterior_strata`, which synchronises the stream.  What is
    wrong raises ValueError before the library is loaded or a graph handle is made."""
    who = "posterior_strata_mc"
    a = _McSweep(who, graph, beta, gamma, sims, maxTime, candidates, "seed", start, shifts, sim_offset)
    now, hz, hz32 = _mc_horizons(who, now, horizons, a.T)
    M = _whole(who, "mismatches", mismatches, 0)
    if M > SIR_POST_MAXD - 1:
        raise ValueError(f"{who}: mismatches = {M} is not in [0, {SIR_POST_MAXD - 1}]")
    squeezed, sets = _timed_records(who, observations, a.n)
    O, H, D = len(sets), int(hz.size), M + 1
    counts, accepted = a.launch("gnode_sir_mc_philox_sweep_posterior_strata", "gnode_sir_sweep_posterior_workspace_bytes",
                                [("counts", counts, (O, D, H, 2, a.n)), ("accepted", accepted, (O, a.C, D))], rng_seed, edge_scan, device,
                                evidence=sets, group=SIR_SCORE_MAXO, scalars=(now, _lib.host_ptr(hz32), H, M), query_scalars=(H,),
                                cells=("count", "fewer horizons or mismatches"))
    return SirPosteriorStrata(counts, accepted, a.sims, now, tuple(int(h) for h in hz), tuple(len(s[0]) for s in sets), squeezed)


def sir_counts_counted(graph: DeviceGraph, seed_set, beta, gamma, sims, T, rng_seed, sim_offset=0, device="cuda"):
    """`sir_counts` through the kernel's profiling instantiation: (counts, stats) with stats = what the launch did --
    Philox blocks computed, infection coins drawn, recovery coins drawn, CSR entries read (bench.py's `sir` roofline)."""
    st = (C.c_uint64 * 4)()
    counts = torch.zeros((3, T, graph.n), dtype=torch.int32, device=device)
    _sir_launch(graph, seed_set, beta, gamma, sims, T, rng_seed, sim_offset, None, None, counts, False, "gnode_sir_mc_philox_counted", (st,))
    return counts, {"philox_blocks": int(st[0]), "infection_coins": int(st[1]), "recovery_coins": int(st[2]), "csr_entries_read": int(st[3])}


def _counts_f64(counts: torch.Tensor) -> np.ndarray:
    """The kernels' uint32 counts (held in an int32 tensor) as float64 on the host."""
    return (counts.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).astype(np.float64)


def sir_counts_coins(n, table: np.ndarray, seed_set, beta, gamma, sims, T, coins: np.ndarray, device="cuda"):
    """Parity mode: consume a recorded torch.rand stream exactly like the reference.
    Returns (counts int32 [3,T,n] on the GPU, coins consumed)."""
    lib = _lib.load()
    seeds = np.ascontiguousarray(list(seed_set), dtype=np.int32)
    tsrc = torch.from_numpy(np.ascontiguousarray(table[:, 0], dtype=np.int32)).to(device)
    tdst = torch.from_numpy(np.ascontiguousarray(table[:, 1], dtype=np.int32)).to(device)
    cz = torch.from_numpy(np.ascontiguousarray(coins, dtype=np.float64)).to(device)
    counts = torch.zeros((3, T, n), dtype=torch.int32, device=device)
    ws = torch.empty(lib.gnode_sir_coins_workspace_bytes(), dtype=torch.uint8, device=device)
    used = C.c_int64(0)
    _lib.check(lib.gnode_sir_mc_coins(_lib.ptr(tsrc), _lib.ptr(tdst), int(tsrc.numel()), int(n), _lib.host_ptr(seeds),
                                      int(seeds.shape[0]), float(beta), float(gamma), int(sims), int(T),
                                      _lib.ptr(cz) if cz.numel() else None, int(cz.numel()), _lib.ptr(counts),
                                      C.byref(used), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    return counts, int(used.value)


def sir_torch(G, seed_set, beta, gamma, sims=10000, T=20, rng_seed=None, coins=None, normalize_t0=False):
    """Monte-Carlo SIR label generator, reference ode_nn.py:30-88.

    Returns (S, I, R) numpy float64 COUNTS of shape [1, T, n] exactly like the
    reference (callers divide by `sims`, ode_nn_ngraph_sim.py:199); row 0 of S and
    I holds the initial state once (the reference assigns it, :55-56).

    Coins: by default counter-based Philox keyed by (edge|node, step, sim), seeded
    from torch's CPU generator so `torch.manual_seed` governs reproducibility as it
    does for the reference's `torch.rand` (:65,:70).  `coins=` (a recorded stream)
    switches to the bit-exact parity mode.

    normalize_t0 (extension): the reference ASSIGNS row 0 in every trajectory
    (:55-56) instead of accumulating it, so after the caller's `/sims` that row reads 1/sims, not 1 (the loss
    skips t = 0, so it is invisible there).  False (default) reproduces the reference's counts exactly;
    True scales row 0 by `sims` so that counts/sims is the initial state itself.

    Per-node rates (extension): in production mode beta and gamma may each be an array of length n indexed by node id
    (see `sir_counts`), and beta an `EdgeRates` made by `edge_rates(G, M)`: one probability per directed contact.  The
    recorded-stream parity mode takes numbers only.

    Initial-state distributions (extension): in production mode seed_set may be an `InitialState` (see `sir_counts`); row 0
    is then accumulated over the trajectories and normalize_t0 has nothing to do.
    """
    n = G.number_of_nodes()
    if coins is not None:
        if isinstance(beta, RateSchedule) or isinstance(gamma, RateSchedule):
            raise ValueError("sir_torch(coins=...): the parity mode takes scalar beta and gamma, not a RateSchedule")
        if isinstance(seed_set, InitialState):
            raise ValueError("sir_torch(coins=...): the parity mode takes a seed list, not an InitialState")
        if isinstance(beta, EdgeRates) or _node_rates("beta", beta, n) is not None or _node_rates("gamma", gamma, n) is not None:
            raise ValueError("sir_torch(coins=...): the parity mode takes scalar beta and gamma, not per-node arrays or EdgeRates")
        e = _edge_arrays(G)
        table = np.empty((2 * e.shape[0], 2), dtype=np.int64)     # reference :32-38
        table[0::2, 0], table[0::2, 1] = e[:, 0], e[:, 1]
        table[1::2, 0], table[1::2, 1] = e[:, 1], e[:, 0]
        counts, _ = sir_counts_coins(n, table, seed_set, beta, gamma, sims, T, np.asarray(coins))
    else:
        if rng_seed is None:
            rng_seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())
        counts = sir_counts(_device_graph_for(G), seed_set, beta, gamma, sims, T, rng_seed)
    c = _counts_f64(counts)
    if normalize_t0 and not isinstance(seed_set, InitialState):     # (a drawn start: row 0 already holds counts)
        c[:, 0] *= float(sims)
    return c[0][None], c[1][None], c[2][None]


def get_sir_t_nodes_torch(x_rk, maxTime, deltaT, count=True):
    """Row subsample out[i] = x[int(i/deltaT)], reference ode_nn.py:249-261.
    One device-side index_select instead of maxTime D2H row copies; the result stays
    on x_rk's device (the reference builds it on the CPU and callers move it back,
    ode_nn_ngraph_sim.py:234)."""
    idx = torch.as_tensor([int(i / deltaT) for i in range(int(maxTime))], device=x_rk.device)
    if count:
        return torch.sum(x_rk, axis=1).index_select(0, idx)
    return x_rk.index_select(0, idx)


def sir(x, y, A, beta, gamma):
    """Mean-field RHS, reference ode_nn.py:214-220 (numpy; kept for callers that pass it to `runge_kutta_order4`)."""
    n = np.shape(A)[0]
    S, I = x[:n], x[n:2 * n]
    AI = np.asarray(A @ I).reshape(-1)
    dS = -beta * AI * S
    return np.hstack([dS, -dS - gamma * I, gamma * I])


def _is_number(v) -> bool:
    return (v.ndim == 0) if isinstance(v, torch.Tensor) else (not isinstance(v, EdgeRates) and np.ndim(v) == 0)


def _mf_rate_rows(name: str, value, n: int, B: int, batch: bool):
    """`value` as float64 [B, n] host rows of mean-field RATES: finite and >= 0, not probabilities (the mean-field takes
    rates, and beta * degree > 1 is ordinary).  A number, per-node rates [n], and with `batch` also [B, n] or B numbers, one
    per sample (a 1-D value of length n is per node, also where B == n).  Raises ValueError before any library call."""
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0 or a.shape == (n,) or (batch and a.shape == (B, n)):
        rows = np.broadcast_to(a, (B, n))
    elif batch and a.shape == (B,):
        rows = np.broadcast_to(a[:, None], (B, n))
    else:
        forms = f"({n},), ({B}, {n}) or ({B},)" if batch else f"({n},)"
        raise ValueError(f"{name}: rates must be a number or have shape {forms}, got {tuple(a.shape)}")
    bad = np.argwhere(~((rows >= 0.0) & np.isfinite(rows)))         # a NaN fails the comparison
    if bad.size:
        b, v = int(bad[0][0]), int(bad[0][1])
        raise ValueError(f"{name}: the rate of sample {b}, node {v}, {rows[b, v]}, is not a finite rate >= 0")
    return np.array(rows, dtype=np.float64)                         # a writable, contiguous copy of the broadcast


def _mf_times(deltaT, maxTime):
    grid = np.arange(0, maxTime, deltaT)
    return np.ascontiguousarray([grid[int(i / deltaT)] for i in range(int(maxTime))], dtype=np.float64)


def _mf_checked(n: int, nnz: int, starts, beta, gamma, batch: bool):
    """The host side of one gnode_meanfield_rates_f64 call, checked before the library is entered: (init [B, n, 3], beta
    [B, n] or None, w [nnz] or None, gamma [B, n]).  With an `EdgeRates` the contact rate is w alone and beta is None."""
    B = len(starts)
    if B < 1:
        raise ValueError("meanfield: need at least one start")
    init = np.empty((B, n, 3), dtype=np.float64)
    for b, start in enumerate(starts):
        init[b] = (_init_for(start, n) if isinstance(start, InitialState) else InitialState.from_sets(n, list(start))).p
    if isinstance(beta, EdgeRates):
        if (beta.n, beta.nnz) != (n, nnz):
            raise ValueError(f"EdgeRates of a graph with {beta.n} nodes / {beta.nnz} entries given for one with {n} / {nnz}")
        b_rows, w = None, beta.w
    else:
        b_rows, w = _mf_rate_rows("beta", beta, n, B, batch), None
    return init, b_rows, w, _mf_rate_rows("gamma", gamma, n, B, batch)


def _meanfield_rates(graph: DeviceGraph, args, t_out, rtol, atol):
    """One gnode_meanfield_rates_f64 call for what `_mf_checked` returned: (out, steps), out a float64 device tensor
    [3 = (I, S, R), len(t_out), B * n] with row b * n + node."""
    init, b_rows, w, g_rows = args
    B, n = init.shape[0], init.shape[1]
    lib, handle = _lib.load(), graph.handle
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: None if a is None or a.size == 0 else torch.from_numpy(a).to(dev)      # noqa: E731  (no edge, no table)
    y0, bet, wd, gam = up(init), up(b_rows), up(w), up(g_rows)
    out = torch.empty((3, len(t_out), B * n), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.gnode_meanfield_rates_workspace_bytes(handle, B), dtype=torch.uint8, device=dev)
    steps = C.c_int64(0)
    _lib.check(lib.gnode_meanfield_rates_f64(handle, B, _lib.ptr(y0), _lib.ptr(bet), _lib.ptr(wd), _lib.ptr(gam),
                                             _lib.host_ptr(t_out), int(len(t_out)), float(rtol), float(atol), _lib.ptr(out[0]),
                                             _lib.ptr(out[1]), _lib.ptr(out[2]), C.byref(steps), _lib.ptr(ws), ws.numel(),
                                             _lib.stream_ptr()))
    return out, int(steps.value)


def runge_kutta_order4(sir, A, n_nodes, indices, beta_factor, gamma_factor, deltaT=1, maxTime=70, rtol=1e-10, atol=1e-12):
    """Mean-field baseline, reference ode_nn.py:222-233 (despite its name the reference runs scipy's LSODA):
    returns (I_sampled_t, S_sampled_t, R_sampled_t), float64 [maxTime, n] at the times int(i/deltaT)*deltaT.
    `sir` (the RHS callable) is accepted for signature compatibility; the integration runs in libgnode_hip.so
    (adaptive Dormand-Prince 5(4), sparse A I) -- SURVEY 8f rank 4, not on the `ode_nn` path.
    `indices` is the seed list, or (extension) an `InitialState`: y(0) = (pS, pI, pR).

    Heterogeneous rates (extension, `gnode_meanfield_rates_f64`): beta_factor may be per-node rates of length n, indexed by
    the target node as x[:, 3], or an `EdgeRates` made for A's sorted CSR -- w[p], in row u with col[p] = v, is the rate at
    which u infects v, the contact rate is then w alone, and A's pattern must be symmetric (a directed contact is a zero on
    the reverse entry).  gamma_factor may be per-node rates of length n.  These are RATES, finite and >= 0, not
    probabilities: the mean-field takes rates, and the reference's own configurations have beta * degree > 1.  A wrong
    length, a NaN, a negative value or an `EdgeRates` of another graph raises ValueError before the library is loaded.  Two
    numbers take the scalar entries as before.  A's stored values are ignored in every form."""
    refuse_schedule("runge_kutta_order4", beta_factor=beta_factor, gamma_factor=gamma_factor)
    Ac = sp.csr_matrix(A)
    Ac.sort_indices()
    n = Ac.shape[0]
    if isinstance(indices, InitialState):
        _init_for(indices, n)
    if not (_is_number(beta_factor) and _is_number(gamma_factor)):
        args = _mf_checked(n, int(Ac.nnz), [indices], beta_factor, gamma_factor, batch=False)
        g = DeviceGraph(Ac.indptr.astype(np.int32), Ac.indices.astype(np.int32))
        o = _meanfield_rates(g, args, _mf_times(deltaT, maxTime), rtol, atol)[0].cpu().numpy()
        return o[0], o[1], o[2]
    lib = _lib.load()
    g = DeviceGraph(Ac.indptr.astype(np.int32), Ac.indices.astype(np.int32))
    t_out = _mf_times(deltaT, maxTime)
    dev = torch.device("cuda", torch.cuda.current_device())
    gam = torch.full((n,), float(gamma_factor), dtype=torch.float64, device=dev)
    out = torch.empty((3, len(t_out), n), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.gnode_meanfield_workspace_bytes(g.handle), dtype=torch.uint8, device=dev)
    steps = C.c_int64(0)
    tail = (float(beta_factor), _lib.ptr(gam), _lib.host_ptr(t_out), int(len(t_out)), float(rtol), float(atol), _lib.ptr(out[0]),
            _lib.ptr(out[1]), _lib.ptr(out[2]), C.byref(steps), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    if isinstance(indices, InitialState):                           # y(0) = (pS, pI, pR)
        y0 = torch.from_numpy(indices.p).to(dev)
        _lib.check(lib.gnode_meanfield_init_f64(g.handle, _lib.ptr(y0), *tail))
    else:
        seeds = np.ascontiguousarray(list(indices), dtype=np.int32)
        _lib.check(lib.gnode_meanfield_f64(g.handle, _lib.host_ptr(seeds), int(seeds.shape[0]), *tail))
    o = out.cpu().numpy()
    return o[0], o[1], o[2]


class MeanfieldBatch(NamedTuple):
    I: torch.Tensor
    S: torch.Tensor
    R: torch.Tensor


def meanfield_batch(graph: DeviceGraph, starts, beta, gamma, deltaT=1, maxTime=70, rtol=1e-10, atol=1e-12) -> MeanfieldBatch:
    """The mean-field baseline for B samples on one graph in ONE integration (`gnode_meanfield_rates_f64`): (I, S, R),
    float64 device tensors [B, maxTime, n] at `runge_kutta_order4`'s times.

    starts: B seed lists and / or `InitialState`s.  beta: a number, per-node rates [n] (indexed by the target node),
    [B, n], B numbers (one per sample; a 1-D value of length n is per node), or an `EdgeRates` of `graph` (the contact
    rate is then w alone).  gamma: a number, [n], [B, n] or B numbers.  Rates are finite and >= 0, not probabilities; what
    is wrong raises ValueError before the library is entered.

    The B samples share the launches, the host round trip per step and the step size: the error norm is the maximum over
    every sample, so a sample's numbers differ from its solo `runge_kutta_order4` run at the level of rtol / atol, not bit
    for bit."""
    refuse_schedule("meanfield_batch", beta=beta, gamma=gamma)
    starts = list(starts)
    n, B = int(graph.n), len(starts)
    out, _ = _meanfield_rates(graph, _mf_checked(n, int(graph.nnz), starts, beta, gamma, batch=True), _mf_times(deltaT, maxTime),
                              rtol, atol)
    I, S, R = (out[c].view(-1, B, n).permute(1, 0, 2).contiguous() for c in range(3))
    return MeanfieldBatch(I, S, R)


class _MeanfieldMarginals(torch.autograd.Function):
    """gnode_meanfield_rates_steps_f64 forward, gnode_meanfield_rates_backward_f64 backward; the arguments are
    `meanfield_marginals`', already checked and expanded to the library's shapes (beta and w may be None)."""

    @staticmethod
    def forward(ctx, graph, init, beta, gamma, w, t_out, rtol, atol):
        lib, handle = _lib.load(), graph.handle
        det = lambda t: None if t is None else t.detach().contiguous()      # noqa: E731
        y0, bet, gam, wd = det(init), det(beta), det(gamma), det(w)
        B, n, T = y0.shape[0], y0.shape[1], len(t_out)
        out = torch.empty((3, T, B * n), dtype=torch.float64, device=y0.device)
        ws = torch.empty(lib.gnode_meanfield_rates_workspace_bytes(handle, B), dtype=torch.uint8, device=y0.device)
        steps, n_h, n_acc, cap = C.c_int64(0), C.c_int64(0), np.zeros(T, dtype=np.int32), 4096
        while True:                                                 # once more, with room, if the record did not fit
            h = np.empty(cap, dtype=np.float64)
            _lib.check(lib.gnode_meanfield_rates_steps_f64(
                handle, B, _lib.ptr(y0), _lib.ptr(bet), _lib.ptr(wd), _lib.ptr(gam), _lib.host_ptr(t_out), T, float(rtol), float(atol),
                _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), C.byref(steps), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(),
                _lib.host_ptr(h), cap, C.byref(n_h), _lib.host_ptr(n_acc)))
            if n_h.value <= cap:
                break
            cap = int(n_h.value)
        ctx.graph, ctx.t_out, ctx.h, ctx.n_acc = graph, t_out, np.ascontiguousarray(h[:n_h.value]), n_acc
        ctx.has = (bet is not None, wd is not None)
        ctx.save_for_backward(*(t for t in (y0, gam, out, bet, wd) if t is not None))
        I, S, R = (out[c].view(T, B, n).permute(1, 0, 2).contiguous() for c in range(3))
        return I, S, R

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gI, gS, gR):
        saved = list(ctx.saved_tensors)
        y0, gam, out = saved[:3]
        bet = saved[3] if ctx.has[0] else None
        wd = saved[-1] if ctx.has[1] else None
        graph, t_out = ctx.graph, ctx.t_out
        B, n, T, nnz = y0.shape[0], y0.shape[1], len(t_out), int(graph.nnz)
        gout = torch.zeros((3, T, B * n), dtype=torch.float64, device=y0.device)      # the outputs' layout: [T][B * n]
        for c, g in enumerate((gI, gS, gR)):
            if g is not None:
                gout[c].view(T, B, n).copy_(g.permute(1, 0, 2))
        want_i, want_b, want_g, want_w = (ctx.needs_input_grad[k] for k in (1, 2, 3, 4))
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=y0.device)      # noqa: E731
        gi, gb = new(B, n, 3) if want_i else None, new(B, n) if want_b and bet is not None else None
        gg = new(B, n) if want_g else None
        gw = new(B, nnz) if want_w and wd is not None and nnz else None      # (no edge, no table: an empty tensor has no address)
        if gi is not None or gb is not None or gg is not None or gw is not None:
            lib, handle = _lib.load(), graph.handle
            m = int(ctx.n_acc.max(initial=0))
            ws = torch.empty(lib.gnode_meanfield_rates_backward_workspace_bytes(handle, B, m), dtype=torch.uint8, device=y0.device)
            _lib.check(lib.gnode_meanfield_rates_backward_f64(
                handle, B, _lib.ptr(y0), _lib.ptr(bet), _lib.ptr(wd), _lib.ptr(gam), _lib.host_ptr(t_out), T, _lib.host_ptr(ctx.h),
                int(ctx.h.shape[0]), _lib.host_ptr(ctx.n_acc), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.ptr(gout[0]),
                _lib.ptr(gout[1]), _lib.ptr(gout[2]), _lib.ptr(gi), _lib.ptr(gb), _lib.ptr(gw), _lib.ptr(gg), _lib.ptr(ws), ws.numel(),
                _lib.stream_ptr()))
        if want_w and wd is not None:                               # the library returns one row per sample: the shared table sums them
            gw = torch.zeros_like(wd) if gw is None else gw.sum(0)
        return None, gi, gb, gg, gw, None, None, None


def meanfield_marginals(graph: DeviceGraph, init, beta, gamma, w=None, deltaT=1, maxTime=70, rtol=1e-10, atol=1e-12) -> MeanfieldBatch:
    """The mean-field marginals of B samples on one graph as a differentiable function of float64 device tensors: (I, S, R),
    [B, maxTime, n] each, bit for bit what `meanfield_batch` returns for the same numbers, with `.backward()` through the
    library's reverse sweep of the Dormand-Prince solve (gnode_meanfield_rates_backward_f64) -- fitting beta and gamma to
    observed curves, per-contact rates, scoring source nodes by the gradient with respect to the start.  The gradient is
    the exact derivative of the returned numbers with the accepted step sizes held fixed (what backpropagating through an
    explicit dopri5 loop gives), not a continuous adjoint.

    init: [B, n, 3] = (pS, pI, pR) per node.  beta: [B, n], [n] (indexed by the target node) or None = 1.  gamma: [B, n] or
    [n].  w: [nnz] in the graph's CSR position order (source = row, target = column; the pattern must then be symmetric) or
    None = 1.  The [n] forms are expanded in front of the library call, so their gradient is the sum over the samples, as w's
    is.  What is wrong raises ValueError before the library is loaded; a tensor that is not on a GPU raises GnodeError."""
    refuse_schedule("meanfield_marginals", beta=beta, gamma=gamma, w=w)
    n, nnz, T = int(graph.n), int(graph.nnz), int(maxTime)
    if T < 1:
        raise ValueError(f"meanfield_marginals: maxTime must be >= 1 (got {maxTime})")
    if not deltaT > 0:
        raise ValueError(f"meanfield_marginals: deltaT must be > 0 (got {deltaT})")
    for name, t in (("init", init), ("beta", beta), ("gamma", gamma), ("w", w)):
        if t is None and name in ("beta", "w"):
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
            raise ValueError(f"meanfield_marginals: {name} must be a float64 tensor")
    if init.dim() != 3 or init.shape[0] < 1 or tuple(init.shape[1:]) != (n, 3):
        raise ValueError(f"meanfield_marginals: init must have the shape [B >= 1, {n}, 3], got {tuple(init.shape)}")
    B = init.shape[0]
    if beta is not None and tuple(beta.shape) not in ((n,), (B, n)):
        raise ValueError(f"meanfield_marginals: beta must have the shape [{n}] or [{B}, {n}], got {tuple(beta.shape)}")
    if tuple(gamma.shape) not in ((n,), (B, n)):
        raise ValueError(f"meanfield_marginals: gamma must have the shape [{n}] or [{B}, {n}], got {tuple(gamma.shape)}")
    if w is not None and tuple(w.shape) != (nnz,):
        raise ValueError(f"meanfield_marginals: w must have the shape [{nnz}], got {tuple(w.shape)}")
    if 3 * B * n >= 2**31:
        raise ValueError(f"meanfield_marginals: 3 * B * n = {3 * B * n} does not fit 31 bits")
    for t in (init, beta, gamma, w):
        if t is not None and not t.is_cuda:
            raise _lib.GnodeError("GN-ODE path: tensor is not on a GPU (no CPU fallback exists)")
    if beta is not None and beta.dim() == 1:
        beta = beta.unsqueeze(0).expand(B, n)                       # autograd sums the samples' rows
    if gamma.dim() == 1:
        gamma = gamma.unsqueeze(0).expand(B, n)
    if w is not None and nnz == 0:
        w = None                                                    # (no edge, no table)
    return MeanfieldBatch(*_MeanfieldMarginals.apply(graph, init, beta, gamma, w, _mf_times(deltaT, T), rtol, atol))


class CsrGraph:
    """What the path needs from the reference's networkx graph, restored from the CSR cache file: node count,
    the edge list in `G.edges()` iteration order (sir_torch's table order, ode_nn.py:32-38) and the adjacency."""

    def __init__(self, n, edges):
        self._n, self.edge_array = int(n), np.ascontiguousarray(edges, dtype=np.int64).reshape(-1, 2)

    def number_of_nodes(self):
        return self._n

    def number_of_edges(self):
        return int(self.edge_array.shape[0])

    def edges(self):
        return [tuple(e) for e in self.edge_array.tolist()]

    def nodes(self):
        return range(self._n)


CACHE_SUFFIX = ".gnode-csr.npz"


def create_graph(n_nodes, graph_label="none", cache=False):
    """reference ode_nn.py:394-414: pickled networkx graph -> undirected -> largest
    connected component -> scipy adjacency.  Returns (G, A, 0).

    cache=True (extension): keep `<graph_label>.gnode-csr.npz` next to the pickle -- node count,
    edge list in `G.edges()` order, CSR of the adjacency -- and, when it is at least as new as the pickle, ingest
    from it without unpickling / re-deriving the component and the adjacency (G is then a `CsrGraph`)."""
    import networkx as nx
    if graph_label != "none":
        src, cfile = graph_label + ".pkl", graph_label + CACHE_SUFFIX
        if cache and os.path.exists(cfile) and os.path.getmtime(cfile) >= os.path.getmtime(src):
            z = np.load(cfile, allow_pickle=False)
            n = int(z["n"])
            A = sp.csr_matrix((z["data"], z["indices"], z["indptr"]), shape=(n, n))
            return CsrGraph(n, z["edges"]), A, 0
        with open(src, "rb") as fh:
            G = pickle.load(fh)
        G = G.to_undirected()
        largest_cc = max(nx.connected_components(G), key=len)
        G = G.subgraph(largest_cc)
    else:
        G = nx.fast_gnp_random_graph(n_nodes, 0.2)
    A = nx.adjacency_matrix(G)
    if cache and graph_label != "none":
        # positions, not labels: the reference indexes tensors with node ids and all its graphs are labelled 0..n-1
        # in node order; anything else is not cacheable in this form
        nodes = list(G.nodes())
        if nodes == list(range(len(nodes))):
            Ac = sp.csr_matrix(A)
            np.savez(graph_label + CACHE_SUFFIX, n=np.int64(len(nodes)), edges=_edge_arrays(G), data=Ac.data,
                     indices=Ac.indices, indptr=Ac.indptr)
    return G, A, 0
