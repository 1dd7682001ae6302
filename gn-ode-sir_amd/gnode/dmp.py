"""Drop-in for `DMP_SIR` of reference dmp.py:74-170 (the `model='dmp'` comparison column):
same constructor and `run(seed_list, maxTime)`, the message passing runs in libgnode_hip.so.

    DMP_SIR(weight_adj, nodes_gamma)        weight_adj: scipy sparse / dense [n, n] (the reference passes A*beta)
        .run(seed_list, maxTime) -> float32 tensor [maxTime, n, 3] = (Ps, Pi, Pr) on the GPU
                                                seed_list: seed ids, or an `InitialState` (an extension)
    dmp_batch(weight_adj, starts, gamma, maxTime, scale=None) -> float32 tensor [B, maxTime, n, 3] (an extension): B
                                                samples on one graph in one library call, each its solo run's bits
                                                weight_adj, scale and gamma may each be a `gnode.ode_nn.RateSchedule`: rates
                                                that change over time (gnode_dmp_batch_schedule_f32)
    dmp_marginals(DmpGraph, weights, gamma, init, maxTime) -> the same tensor as a torch.autograd.Function of device tensors (an
                                                extension): gradients with respect to weights, gamma and the start
    dmp_marginals_schedule(DmpGraph, weights, gamma, init, maxTime, phase) -> `dmp_batch` under a rate schedule as such a
                                                function (an extension): weights [P, nnz], gamma [P, n] hold one table per
                                                phase, phase names each step's, and `.backward()` fills every phase's gradient
    source_scores(graph, obs, gamma, maxTime, candidates=None, floor=1e-30, budget_bytes=1 << 30) -> float64 tensor
                                                [C, maxTime] on the GPU (an extension): the log-likelihood of one observed
                                                snapshot for every candidate source and time, fused into the node pass
    rank_sources(scores, candidates)         -> the candidates by their best score, with the time at which each attains it
    source_scores_batch(graph, obs, gamma, maxTime, candidates=None, floor=1e-30, budget_bytes=1 << 30) -> float64 tensor
                                                [O, C, maxTime] on the GPU (an extension): `source_scores` for O snapshots
                                                [O, n] (a device tensor of `sir_state_at` is used where it lies) in one pass of
                                                the recurrence, row o bit for bit the solo call's; source_candidates_batch(obs)
                                                is its default candidate list
    source_rank_of(scores, candidates, truth) -> int64 tensor [O]: how many candidates beat each snapshot's true source
    source_scores_events(graph, rows, gamma, maxTime, candidates=None, floor=1e-30, budget_bytes=1 << 30) -> float64 tensor
                                                [R, C, maxTime] on the GPU (an extension): `source_scores_batch` with the codes
                                                3 = became infected at the step and 4 = recovered at the step, differences of
                                                consecutive marginals taken in the node pass
    timed_observations(n, nodes, offsets, kinds) -> TimedObservations: records taken at different times, packed into such rows;
                                                observations_from_events(t_inf, t_rec, now, sensors, what) makes the records
    source_scores_timed(graph, observations, gamma, maxTime, ...) -> float64 tensor [C, maxTime]: the log-likelihood of all
                                                records when "now" is t steps after c was seeded (`sum_timed_rows` of the rows)
    outbreak_sizes(graph, gamma, maxTime, candidates=None, action="seed", start=None, value=None, budget_bytes=1 << 30)
                                             -> float64 tensor [C, maxTime, 3] on the GPU (an extension): the expected size of
                                                S / I / R over time when candidate c alone is seeded or immunised in `start`,
                                                summed in the node pass; infections(sizes) -> the number ever infected, [C]
    source_scores_schedule(weight_adj, rows, gamma, maxTime, observed_at=None, ...), outbreak_sizes_schedule(weight_adj, gamma,
                                                maxTime, ..., shifts=None) -> `source_scores_events` and `outbreak_sizes` when
                                                weight_adj, scale and / or gamma is a RateSchedule: per sample a candidate
                                                and a calendar shift; observed_at=D anchors the snapshot at calendar step D
    greedy_immunisation(graph, start, gamma, maxTime, k), greedy_seeds(graph, gamma, maxTime, k, start=None)
                                             -> [(node, infections_after), ...]: k greedy rounds of outbreak_sizes
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from .graph import DeviceGraph


def _refuse_schedule(who, **args):
    from .ode_nn import refuse_schedule
    refuse_schedule(who, **args)


class DMP_SIR:
    def __init__(self, weight_adj, nodes_gamma, device="cuda"):
        _refuse_schedule("DMP_SIR", weight_adj=weight_adj, nodes_gamma=nodes_gamma)
        A = sp.csr_matrix(weight_adj)
        A.sort_indices()
        self.N = A.shape[0]
        self.E = int(A.nnz)
        self.graph = DeviceGraph(A.indptr.astype(np.int32), A.indices.astype(np.int32))
        self.weights = torch.from_numpy(np.ascontiguousarray(A.data, dtype=np.float32)).to(device)
        self.nodes_gamma = torch.as_tensor(np.asarray(nodes_gamma, dtype=np.float32)).to(device)
        if self.nodes_gamma.numel() != self.N:
            raise _lib.GnodeError(f"DMP_SIR: nodes_gamma has {self.nodes_gamma.numel()} entries for {self.N} nodes")
        self.marginals = None

    def run(self, seed_list, maxTime):
        """seed_list: the seed ids, or (extension) a `gnode.ode_nn.InitialState`: Ps_0, Pi_0, Pr_0 are then its columns and
        the messages start from Phi_0 = Pi_0[src] (gnode_dmp_init_f32)."""
        from .ode_nn import InitialState
        if isinstance(seed_list, InitialState) and seed_list.n != self.N:
            raise ValueError(f"InitialState of {seed_list.n} nodes given for a graph of {self.N}")
        lib = _lib.load()
        out = torch.empty((int(maxTime), self.N, 3), dtype=torch.float32, device=self.weights.device)
        if isinstance(seed_list, InitialState):
            init = torch.from_numpy(seed_list.p.astype(np.float32)).to(out.device)
            ws = torch.empty(lib.gnode_dmp_init_workspace_bytes(self.graph.handle), dtype=torch.uint8, device=out.device)
            _lib.check(lib.gnode_dmp_init_f32(self.graph.handle, _lib.ptr(self.weights), _lib.ptr(self.nodes_gamma), _lib.ptr(init),
                                              int(maxTime), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
            self.marginals = out
            return out
        seeds = np.ascontiguousarray(list(seed_list), dtype=np.int32)
        ws = torch.empty(lib.gnode_dmp_workspace_bytes(self.graph.handle), dtype=torch.uint8, device=out.device)
        _lib.check(lib.gnode_dmp_f32(self.graph.handle, _lib.ptr(self.weights), _lib.ptr(self.nodes_gamma), _lib.host_ptr(seeds),
                                     int(seeds.shape[0]), int(maxTime), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                     _lib.stream_ptr()))
        self.marginals = out
        return out

    def output(self):
        return self.marginals


class DmpGraph:
    """One weighted adjacency prepared for several `dmp_batch` calls: the sorted CSR on the host, and the graph handle, made
    on first use and kept.  `dmp_batch` takes it wherever it takes a matrix."""

    def __init__(self, weight_adj):
        _refuse_schedule("DmpGraph", weight_adj=weight_adj)
        A = sp.csr_matrix(weight_adj)
        A.sort_indices()
        self.N, self.E = int(A.shape[0]), int(A.nnz)
        self.indptr, self.indices = A.indptr.astype(np.int32), A.indices.astype(np.int32)
        self.data = np.ascontiguousarray(A.data, dtype=np.float64)
        self._graph = None

    @property
    def graph(self):
        if self._graph is None:
            self._graph = DeviceGraph(self.indptr, self.indices)
        return self._graph


class _DmpMarginals(torch.autograd.Function):
    """gnode_dmp_batch_f32 forward, gnode_dmp_batch_backward_f32 backward; with `phase` (an int32 host array [maxTime]) their
    scheduled counterparts, gnode_dmp_batch_schedule_f32 and gnode_dmp_batch_schedule_backward_f32, whose tables hold P phases
    each: [P, nnz] and [P, n] where the constant call has [nnz] and [n].  The arguments are `dmp_marginals`' or
    `dmp_marginals_schedule`'s, already checked."""

    @staticmethod
    def _rates(w, g, n, nnz, phase):
        """The leading arguments of both entries after the handle -- the tables, their per-sample strides and, under a schedule,
        the phase row and P -- of the tensors at hand (a pointer is only as good as the tensor it was taken from), and the phases
        of a table as a shape: () or (P,)."""
        tables = () if phase is None else (int(g.shape[-2]),)       # between a table's sample and its entries
        P, shared = int(np.prod(tables)), 1 + len(tables)           # a table of `shared` dimensions serves every sample: stride 0
        rates = (_lib.ptr(w) if nnz else None, 0 if w.dim() == shared else P * nnz, _lib.ptr(g), 0 if g.dim() == shared else P * n)
        return rates + (() if phase is None else (_lib.host_ptr(phase), P)), tables

    @staticmethod
    def forward(ctx, graph, weights, gamma, init, maxTime, phase):
        lib, handle = _lib.load(), graph.graph.handle
        w, g, y0 = weights.detach().contiguous(), gamma.detach().contiguous(), init.detach().contiguous()
        B, n, nnz = y0.shape[0], graph.N, graph.E
        rates, _ = _DmpMarginals._rates(w, g, n, nnz, phase)
        out = torch.empty((B, maxTime, n, 3), dtype=torch.float32, device=y0.device)
        if phase is None:
            entry, need = lib.gnode_dmp_batch_f32, lib.gnode_dmp_batch_workspace_bytes(handle, B)
        else:
            entry, need = lib.gnode_dmp_batch_schedule_f32, lib.gnode_dmp_batch_schedule_workspace_bytes(handle, B, maxTime)
        ws = torch.empty(need, dtype=torch.uint8, device=y0.device)
        _lib.check(entry(handle, *rates, _lib.ptr(y0), B, maxTime, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        ctx.graph, ctx.maxTime, ctx.phase = graph, maxTime, phase
        ctx.save_for_backward(w, g, y0, out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        w, g, y0, out = ctx.saved_tensors
        graph, T, grad_out = ctx.graph, ctx.maxTime, grad_out.contiguous()
        B, n, nnz = y0.shape[0], graph.N, graph.E
        want_w, want_g, want_i = ctx.needs_input_grad[1:4]
        rates, tables = _DmpMarginals._rates(w, g, n, nnz, ctx.phase)        # of the saved tensors as autograd hands them back
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=y0.device)      # noqa: E731
        gw = new(B, *tables, nnz) if want_w and nnz else None        # (no edge, no table: an empty tensor has no address)
        gg, gi = new(B, *tables, n) if want_g else None, new(B, n, 3) if want_i else None
        if gw is not None or gg is not None or gi is not None:
            lib, handle = _lib.load(), graph.graph.handle
            if ctx.phase is None:
                entry, need = lib.gnode_dmp_batch_backward_f32, lib.gnode_dmp_batch_backward_workspace_bytes(handle, B, T)
            else:
                entry, need = lib.gnode_dmp_batch_schedule_backward_f32, lib.gnode_dmp_batch_schedule_backward_workspace_bytes(handle, B, T)
            ws = torch.empty(need, dtype=torch.uint8, device=y0.device)
            _lib.check(entry(handle, *rates, _lib.ptr(y0), B, T, _lib.ptr(out), _lib.ptr(grad_out), _lib.ptr(gw), _lib.ptr(gg),
                             _lib.ptr(gi), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        if want_w:                                                  # the library returns one block per sample: a shared table sums them
            gw = torch.zeros_like(w) if gw is None else gw.sum(0) if w.dim() == 1 + len(tables) else gw
        if want_g and g.dim() == 1 + len(tables):
            gg = gg.sum(0)
        return None, gw, gg, gi, None, None


def dmp_marginals(graph, weights, gamma, init, maxTime):
    """The DMP marginals of B samples on one graph as a differentiable function of device tensors: float32 [B, maxTime, n, 3] =
    (Ps, Pi, Pr), bit for bit what `dmp_batch` returns for the same numbers, with `.backward()` through the library's reverse
    sweep (gnode_dmp_batch_backward_f32) -- fitting per-contact transmission probabilities and recovery rates to observed
    curves, scoring source nodes by the gradient with respect to the start.

    graph: a `DmpGraph` (only its pattern is read).  weights: float32 [nnz], shared by the samples, or [B, nnz], in the
    graph's CSR position order (`DmpGraph.data`'s).  gamma: float32 [n] or [B, n].  init: float32 [B, n, 3] = (pS, pI, pR) per
    node.  Gradients are computed for the inputs that require one; a shared table gets the sum over the samples.  Where the
    forward is not finite (a weight of 1 next to a seed) the gradient is unspecified.  What is wrong raises ValueError
    before the library is loaded; a tensor that is not on a GPU raises GnodeError."""
    _refuse_schedule("dmp_marginals", graph=graph, weights=weights, gamma=gamma)
    if not isinstance(graph, DmpGraph):
        raise ValueError(f"dmp_marginals: graph must be a DmpGraph, got {type(graph).__name__}")
    T, n, nnz = int(maxTime), graph.N, graph.E
    if T < 2:
        raise ValueError(f"dmp_marginals: maxTime must be >= 2 (got {maxTime})")
    for name, t in (("weights", weights), ("gamma", gamma), ("init", init)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"dmp_marginals: {name} must be a float32 tensor")
    if init.dim() != 3 or init.shape[0] < 1 or tuple(init.shape[1:]) != (n, 3):
        raise ValueError(f"dmp_marginals: init must have the shape [B >= 1, {n}, 3], got {tuple(init.shape)}")
    B = init.shape[0]
    if tuple(weights.shape) not in ((nnz,), (B, nnz)):
        raise ValueError(f"dmp_marginals: weights must have the shape [{nnz}] or [{B}, {nnz}], got {tuple(weights.shape)}")
    if tuple(gamma.shape) not in ((n,), (B, n)):
        raise ValueError(f"dmp_marginals: gamma must have the shape [{n}] or [{B}, {n}], got {tuple(gamma.shape)}")
    for t in (weights, gamma, init):
        if not t.is_cuda:
            raise _lib.GnodeError("GN-ODE path: tensor is not on a GPU (no CPU fallback exists)")
    return _DmpMarginals.apply(graph, weights, gamma, init, T, None)


def dmp_marginals_schedule(graph, weights, gamma, init, maxTime, phase):
    """`dmp_marginals` with rates that change over time: the DMP marginals of B samples under a piecewise-constant schedule of
    P phases as a differentiable function of device tensors -- float32 [B, maxTime, n, 3], bit for bit what `dmp_batch` returns
    for the same schedule -- with `.backward()` through the library's scheduled reverse sweep
    (gnode_dmp_batch_schedule_backward_f32): how strong was the lockdown, did recovery speed up once testing began.

    graph: a `DmpGraph` (only its pattern is read).  weights: float32 [P, nnz], shared by the samples, or [B, P, nnz]: one
    table per phase in the graph's CSR position order.  gamma: float32 [P, n] or [B, P, n], with the same P.  init: float32
    [B, n, 3].  phase: a sequence of whole numbers of length >= maxTime, phase[t] in [0, P) naming the tables of step t = 1 ..
    maxTime-1 (entry 0 is ignored), or a `gnode.ode_nn.RateSchedule`, of which `phase_of_step(maxTime)` is taken and the values
    ignored.  The tables are probabilities: the library refuses a NaN or an entry outside [0, 1] (GnodeError).  Gradients are
    computed for the inputs that require one; a shared table gets the sum over the samples, and a phase no step names gets
    exact zeros.  Step t's phi reads step t's tables and theta_{t+1} the weight of step t + 1, so phase p's weight gradient
    collects both kinds of term.

    One scale per phase needs no kernel of its own: write `weights = base[None, :] * s[:, None]` in torch and autograd carries
    the table's gradient to `s`.  What is wrong raises ValueError before the library is loaded; a tensor that is not on a GPU
    raises GnodeError."""
    from .ode_nn import RateSchedule
    who = "dmp_marginals_schedule"
    _refuse_schedule(who, graph=graph, weights=weights, gamma=gamma)
    if not isinstance(graph, DmpGraph):
        raise ValueError(f"{who}: graph must be a DmpGraph, got {type(graph).__name__}")
    try:
        T = int(maxTime)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: maxTime must be a whole number >= 2 (got {maxTime!r})") from None
    n, nnz = graph.N, graph.E
    if T < 2:
        raise ValueError(f"{who}: maxTime must be >= 2 (got {maxTime})")
    for name, t in (("weights", weights), ("gamma", gamma), ("init", init)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{who}: {name} must be a float32 tensor")
    if init.dim() != 3 or init.shape[0] < 1 or tuple(init.shape[1:]) != (n, 3):
        raise ValueError(f"{who}: init must have the shape [B >= 1, {n}, 3], got {tuple(init.shape)}")
    B = init.shape[0]
    if gamma.dim() not in (2, 3) or gamma.shape[-2] < 1 or gamma.shape[-1] != n or (gamma.dim() == 3 and gamma.shape[0] != B):
        raise ValueError(f"{who}: gamma must have the shape [P >= 1, {n}] or [{B}, P, {n}], got {tuple(gamma.shape)}")
    P = int(gamma.shape[-2])
    if tuple(weights.shape) not in ((P, nnz), (B, P, nnz)):
        raise ValueError(f"{who}: weights must have the shape [{P}, {nnz}] or [{B}, {P}, {nnz}] -- gamma holds P = {P} phases --, got "
                         f"{tuple(weights.shape)}")
    if isinstance(phase, RateSchedule):
        steps = phase.phase_of_step(T).astype(np.int64)              # (a schedule given as too few `steps`: ValueError)
    else:
        steps = _source_ints("phase", phase, who=who)
        if steps.shape[0] < T:
            raise ValueError(f"{who}: phase names {steps.shape[0]} steps, the call has maxTime = {T}")
    steps = steps[:T].copy()
    steps[0] = 0                                                    # never read
    if steps.min() < 0 or steps.max() >= P:
        t_bad = int(np.flatnonzero((steps < 0) | (steps >= P))[0])
        raise ValueError(f"{who}: phase[{t_bad}] = {int(steps[t_bad])} is not in [0, {P})")
    for t in (weights, gamma, init):
        if not t.is_cuda:
            raise _lib.GnodeError("GN-ODE path: tensor is not on a GPU (no CPU fallback exists)")
    return _DmpMarginals.apply(graph, weights, gamma, init, T, np.ascontiguousarray(steps, dtype=np.int32))


def _batch_numbers(name, value, shapes, who="dmp_batch"):
    """`value` as a float64 host array of one of `shapes`, every entry finite and >= 0; ValueError otherwise."""
    _refuse_schedule(who, **{name: value})
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    try:
        a = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{who}: {name} is not an array of numbers ({e})") from None
    if a.shape not in shapes:
        raise ValueError(f"{who}: {name} must have one of the shapes {shapes}, got {tuple(a.shape)}")
    if not ((a >= 0.0) & np.isfinite(a)).all():                     # a NaN fails the comparison
        raise ValueError(f"{who}: {name} holds an entry that is not a finite number >= 0")
    return a


def dmp_batch(weight_adj, starts, gamma, maxTime, scale=None, device="cuda"):
    """`DMP_SIR.run` for B samples on one graph in ONE library call (`gnode_dmp_batch_f32`): a float32 device tensor
    [B, maxTime, n, 3] = (Ps, Pi, Pr).  DMP is a fixed recurrence and no sample reads another's numbers, so row b is bit for bit
    what `DMP_SIR(weight_adj * scale[b], gamma_b).run(starts[b], maxTime)` returns.

    weight_adj: one matrix, as `DMP_SIR` takes, or a `DmpGraph` made from one (its graph handle then serves every call).
    starts: B seed lists and / or `InitialState`s.  scale: None -- the B samples share the matrix's weights -- or B numbers:
    sample b's weights are float32(float64(data) * scale[b]).  gamma: a number, per-node values [n], [B, n], or B numbers, one
    per sample (a 1-D value of length n is per node, also where B == n).  gamma and scale are finite and >= 0.  What is wrong
    raises ValueError before the library is loaded or a graph handle is made.

    Rates that change over time: weight_adj, scale and / or gamma may be a `gnode.ode_nn.RateSchedule` (from `rate_schedule`);
    step t of the recurrence then reads the tables that govern step t, and theta_{t+1} the weight of step t + 1
    (`gnode_dmp_batch_schedule_f32`).  scale's values are each None, a number or B numbers; gamma's are each what gamma
    accepts; weight_adj's are matrices that share one sparsity pattern after `sp.csr_matrix(...).sort_indices()` (an entry
    absent in some phases is stored as an explicit zero there), else ValueError.  The schedules need not change at the same
    steps.  Sample b's weights in a phase are float32(float64(data_p) * scale_p[b]); a schedule of one value returns the
    constant call's bits."""
    from .ode_nn import InitialState, RateSchedule
    if any(isinstance(v, RateSchedule) for v in (weight_adj, scale, gamma)):
        return _dmp_batch_schedule(weight_adj, starts, gamma, maxTime, scale, device)
    G = weight_adj if isinstance(weight_adj, DmpGraph) else DmpGraph(weight_adj)
    starts = list(starts)
    n, nnz, B, T = G.N, G.E, len(starts), int(maxTime)
    if B < 1:
        raise ValueError("dmp_batch: need at least one start")
    if T < 2:
        raise ValueError(f"dmp_batch: maxTime must be >= 2 (got {maxTime})")
    init = _batch_starts(starts, n)
    gam = _batch_gamma(gamma, n, B)
    if scale is None:
        w = G.data.astype(np.float32)
    else:
        sc = _batch_numbers("scale", scale, [(B,)])
        w = (G.data[None, :] * sc[:, None]).astype(np.float32)
    lib, handle = _lib.load(), G.graph.handle
    up = lambda a: None if a.size == 0 else torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731  (no edge, no table)
    wd, gd, y0 = up(w), up(gam), up(init)
    out = torch.empty((B, T, n, 3), dtype=torch.float32, device=y0.device)
    ws = torch.empty(lib.gnode_dmp_batch_workspace_bytes(handle, B), dtype=torch.uint8, device=y0.device)
    _lib.check(lib.gnode_dmp_batch_f32(handle, _lib.ptr(wd), nnz if w.ndim == 2 else 0, _lib.ptr(gd), n if gam.ndim == 2 else 0,
                                       _lib.ptr(y0), B, T, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    return out


def _batch_starts(starts, n):
    """float32 [B, n, 3] of B seed lists and / or `InitialState`s; ValueError for a wrong n or a seed outside the graph."""
    from .ode_nn import InitialState
    init = np.empty((len(starts), n, 3), dtype=np.float32)
    for b, start in enumerate(starts):
        if isinstance(start, InitialState):
            if start.n != n:
                raise ValueError(f"InitialState of {start.n} nodes given for a graph of {n}")
        else:
            start = InitialState.from_sets(n, list(start))          # (a seed outside the graph: ValueError)
        init[b] = start.p.astype(np.float32)
    return init


def _batch_gamma(gamma, n, B, name="gamma", who="dmp_batch"):
    """float32 [n] or [B, n] of what `dmp_batch` accepts as gamma; B None: a number or per-node values only, float32 [n]."""
    g = _batch_numbers(name, gamma, [(), (n,)] if B is None else [(), (n,), (B, n), (B,)], who)
    if B is not None and g.shape == (B,) and g.shape != (n,):
        g = np.repeat(g[:, None], n, axis=1)
    return np.ascontiguousarray(np.broadcast_to(g, (n,)) if g.ndim < 2 else g, dtype=np.float32)


def _schedule_graph(who, weight_adj):
    """(DmpGraph, [float64 data per weight_adj phase]) of a weight_adj that may be a RateSchedule of matrices sharing one sparsity
    pattern; ValueError otherwise."""
    from .ode_nn import RateSchedule
    if not isinstance(weight_adj, RateSchedule):
        G = weight_adj if isinstance(weight_adj, DmpGraph) else DmpGraph(weight_adj)
        return G, [G.data]
    mats = []
    for p, M in enumerate(weight_adj.values):
        if isinstance(M, DmpGraph):
            raise ValueError(f"{who}: weight_adj phase {p}: a schedule takes matrices, not a DmpGraph")
        A = sp.csr_matrix(M)
        A.sort_indices()
        mats.append(A)
    for p, A in enumerate(mats[1:], 1):
        if A.shape != mats[0].shape or not np.array_equal(A.indptr, mats[0].indptr) or not np.array_equal(A.indices, mats[0].indices):
            raise ValueError(f"{who}: weight_adj phase {p} does not share phase 0's sparsity pattern (store an absent entry as an "
                             "explicit zero)")
    return DmpGraph(mats[0]), [np.ascontiguousarray(A.data, dtype=np.float64) for A in mats]


def _schedule_tables(who, G, datas, weight_adj, scale, gamma, L, B=None):
    """The joint phases of the schedules among weight_adj, scale and gamma over a phase row of L entries -- the distinct
    combinations in order of first use -- and their tables: (phase int32 [L], w float32 [P, nnz], gam float32 [P, n]).  With B
    samples that may have rates of their own (`dmp_batch`: a scale of B numbers, gamma [B, n] or B numbers) a table is
    [B, P, ...] where some phase is per sample; B None: the tables are shared, and a scale is None or one number.  Every table
    holds probabilities: a weight times its scale, or a gamma, above 1 raises ValueError, as does a `steps=` schedule shorter
    than L."""
    from .ode_nn import RateSchedule, joint_phases
    n, nnz = G.N, G.E
    s_vals = scale.values if isinstance(scale, RateSchedule) else [scale]
    scales = [None if v is None else _batch_numbers(f"scale phase {p}", v, [()] if B is None else [(), (B,)], who) for p, v in enumerate(s_vals)]
    g_vals = gamma.values if isinstance(gamma, RateSchedule) else [gamma]
    gams = [_batch_gamma(v, n, B, f"gamma phase {p}", who) for p, v in enumerate(g_vals)]
    rows = [s.phase_of_step(L) if isinstance(s, RateSchedule) else np.zeros(L, dtype=np.int32) for s in (weight_adj, scale, gamma)]
    phase, triples = joint_phases(rows)
    P = len(triples)
    per_sample_w = any(scales[ps] is not None and scales[ps].ndim == 1 for _, ps, _ in triples)
    per_sample_g = any(gams[pg].ndim == 2 for _, _, pg in triples)
    w = np.empty((B, P, nnz) if per_sample_w else (P, nnz), dtype=np.float32)
    gam = np.empty((B, P, n) if per_sample_g else (P, n), dtype=np.float32)
    for j, (pw, ps, pg) in enumerate(triples):
        sc = scales[ps]
        table = datas[pw] if sc is None else datas[pw][None, :] * sc[:, None] if sc.ndim == 1 else datas[pw] * sc
        w[..., j, :] = table.astype(np.float32)
        gam[..., j, :] = gams[pg]
        for name, a in (("a weight times its scale", w[..., j, :]), ("gamma", gam[..., j, :])):
            if a.size and a.max() > 1.0:                            # (NaN, infinite and negative values: _batch_numbers)
                raise ValueError(f"{who}: phase {j} (weight_adj {pw}, scale {ps}, gamma {pg}): {name} exceeds 1; a schedule takes "
                                 "probabilities")
    return phase, w, gam


def _dmp_batch_schedule(weight_adj, starts, gamma, maxTime, scale, device):
    """`dmp_batch` where weight_adj, scale and / or gamma is a RateSchedule: the joint phases of the schedules and their tables
    [P][...] (or [B][P][...] where a phase is per sample) from `_schedule_tables`, and one gnode_dmp_batch_schedule_f32 call.
    Everything is checked before the library is loaded or a graph handle is made."""
    who = "dmp_batch"
    starts = list(starts)
    B, T = len(starts), int(maxTime)
    if B < 1:
        raise ValueError("dmp_batch: need at least one start")
    if T < 2:
        raise ValueError(f"dmp_batch: maxTime must be >= 2 (got {maxTime})")
    G, datas = _schedule_graph(who, weight_adj)
    n, nnz = G.N, G.E
    init = _batch_starts(starts, n)
    phase, w, gam = _schedule_tables(who, G, datas, weight_adj, scale, gamma, T, B)
    P, per_sample_w, per_sample_g = int(gam.shape[-2]), w.ndim == 3, gam.ndim == 3
    lib, handle = _lib.load(), G.graph.handle
    up = lambda a: None if a.size == 0 else torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731  (no edge, no table)
    wd, gd, y0 = up(w), up(gam), up(init)
    out = torch.empty((B, T, n, 3), dtype=torch.float32, device=y0.device)
    ws = torch.empty(lib.gnode_dmp_batch_schedule_workspace_bytes(handle, B, T), dtype=torch.uint8, device=y0.device)
    _lib.check(lib.gnode_dmp_batch_schedule_f32(handle, _lib.ptr(wd), P * nnz if per_sample_w else 0, _lib.ptr(gd), P * n if per_sample_g else 0,
                                                _lib.host_ptr(phase), P, _lib.ptr(y0), B, T, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                                _lib.stream_ptr()))
    return out


def _largest_chunk(need, total, budget, who):
    """The largest C <= total whose workspace `need(C)` fits `budget` bytes; ValueError if one candidate does not."""
    if need(1) > budget:
        raise ValueError(f"{who}: budget_bytes = {budget} is too small for one candidate ({need(1)} bytes)")
    lo, hi = 1, total                                               # need(lo) <= budget throughout
    if need(hi) <= budget:
        lo = hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if need(mid) <= budget else (lo, mid)
    return lo


def _source_ints(name, value, n_expected=None, who="source_scores"):
    """`value` as a 1-D int64 host array of whole numbers (of length n_expected, where given); ValueError otherwise."""
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    try:
        a = np.asarray(value)
        if a.dtype.kind not in "iub" and not (a.dtype.kind == "f" and (np.isfinite(a) & (a == np.floor(a))).all()):
            raise ValueError("not whole numbers")
        whole = a.astype(np.int64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{who}: {name} is not an array of integers ({e})") from None
    if whole.ndim != 1 or (n_expected is not None and whole.shape[0] != n_expected):
        want = "1-D" if n_expected is None else f"[{n_expected}]"
        raise ValueError(f"{who}: {name} must have the shape {want}, got {tuple(whole.shape)}")
    return whole


def source_scores(graph, obs, gamma, maxTime, candidates=None, floor=1e-30, budget_bytes=1 << 30, device="cuda"):
    """Which node started the outbreak?  Given ONE observed snapshot `obs` of the SIR states, taken at an unknown time, score
    every candidate source c and time t by the mean-field likelihood of the snapshot under DMP started from c alone (Lokhov,
    Mezard, Ohta, Zdeborova 2014):  scores[c, t] = sum over the observed nodes k of log P^k_{obs[k]}(t | c),  t = 0 .. maxTime - 1,
    a float64 device tensor [C, maxTime].  The probabilities are `dmp_batch`'s float32 marginals from the seed list [c], bit for
    bit, clamped to [floor, 1] in float32 before the float64 logarithm -- a node further than t from c has probability exactly
    0 -- but they never reach global memory: the sums are taken in the node pass that holds them in registers
    (`gnode_dmp_source_scores_f32`), in a fixed order, so a candidate's row does not depend on the other candidates or on the
    chunking.

    graph: one matrix, as `DMP_SIR` takes, or a `DmpGraph` made from one; its `data` gives the weights.  obs: n integers,
    0 / 1 / 2 = observed susceptible / infected / recovered, -1 = not observed.  gamma: a number or per-node values [n], finite
    and >= 0.  candidates: node ids (repeats allowed); by default the nodes observed infected or recovered, ascending -- a source
    cannot be susceptible -- and every node if there is none.  The candidates go to the library in chunks of the largest C
    whose `gnode_dmp_source_workspace_bytes` fits `budget_bytes` (the one-workgroup form needs no room per candidate: one
    chunk); a budget too small for one candidate raises ValueError.  What is wrong raises ValueError before the library is
    loaded or a graph handle is made."""
    G = graph if isinstance(graph, DmpGraph) else DmpGraph(graph)
    n, T = G.N, int(maxTime)
    if T < 2:
        raise ValueError(f"source_scores: maxTime must be >= 2 (got {maxTime})")
    floor = float(floor)
    if not 0.0 < floor <= 1.0 or not 0.0 < float(np.float32(floor)) <= 1.0:        # (a NaN fails it; so does a float32 zero)
        raise ValueError(f"source_scores: floor must be in (0, 1] as a float32 (got {floor})")
    o = _source_ints("obs", obs, n)
    if o.size and (o.min() < -1 or o.max() > 2):
        raise ValueError("source_scores: obs holds a value outside -1 (not observed), 0, 1, 2")
    if candidates is None:
        cand = source_candidates(o)
    else:
        cand = _source_ints("candidates", candidates)
    if cand.size < 1:
        raise ValueError("source_scores: need at least one candidate")
    if cand.min() < 0 or cand.max() >= n:
        raise ValueError(f"source_scores: candidate {int(cand[(cand < 0) | (cand >= n)][0])} is not in [0, {n})")
    g = _batch_numbers("gamma", gamma, [(), (n,)], "source_scores")
    budget = int(budget_bytes)
    lib, handle = _lib.load(), G.graph.handle
    need = lambda c: int(lib.gnode_dmp_source_workspace_bytes(handle, c, T))       # noqa: E731  (grows with c, or is constant)
    chunk = _largest_chunk(need, int(cand.size), budget, "source_scores")
    up = lambda a, dt: None if a.size == 0 else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)      # noqa: E731
    wd, gd = up(G.data, np.float32), up(np.broadcast_to(g, (n,)), np.float32)
    od, cd = up(o, np.int32), up(cand, np.int32)
    scores = torch.empty((cand.size, T), dtype=torch.float64, device=cd.device)
    ws = torch.empty(need(chunk), dtype=torch.uint8, device=cd.device)
    for at in range(0, cand.size, chunk):
        c = min(chunk, cand.size - at)
        _lib.check(lib.gnode_dmp_source_scores_f32(handle, _lib.ptr(wd), _lib.ptr(gd), _lib.ptr(cd[at:at + c]), c, _lib.ptr(od), floor, T,
                                                   _lib.ptr(scores[at:at + c]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    return scores


def source_candidates(obs):
    """The candidates `source_scores` takes by default for `obs`: the nodes observed infected or recovered, ascending; every
    node if there is none."""
    o = np.asarray(obs).astype(np.int64)
    cand = np.flatnonzero(o >= 1)
    return cand if cand.size else np.arange(o.shape[0])


def _is_device_ints(value):
    return isinstance(value, torch.Tensor) and value.is_cuda and not value.dtype.is_floating_point and not value.dtype.is_complex


def _source_obs_rows(obs, n, who, name="obs", top=2):
    """`obs` as O >= 1 rows of n whole numbers in -1 .. top: an integer device tensor stays where it is (checked with torch
    operations), anything else becomes an int64 host array; ValueError otherwise."""
    outside = f"{who}: {name} holds a value outside -1 (not observed), 0 .. {top}"
    if _is_device_ints(obs):
        if obs.dim() != 2 or obs.shape[0] < 1 or obs.shape[1] != n:
            raise ValueError(f"{who}: {name} must have the shape [O >= 1, {n}], got {tuple(obs.shape)}")
        if n and (int(obs.min()) < -1 or int(obs.max()) > top):
            raise ValueError(outside)
        return obs
    if isinstance(obs, torch.Tensor):
        obs = obs.detach().cpu().numpy()
    try:
        a = np.asarray(obs)
    except (TypeError, ValueError) as e:                            # (a ragged list)
        raise ValueError(f"{who}: {name} is not an array of integers ({e})") from None
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != n:
        raise ValueError(f"{who}: {name} must have the shape [O >= 1, {n}], got {tuple(a.shape)}")
    o = _source_ints(name, a.reshape(-1), who=who).reshape(a.shape)
    if o.size and (o.min() < -1 or o.max() > top):
        raise ValueError(outside)
    return o


def source_candidates_batch(obs):
    """The candidates `source_scores_batch` takes by default for the rows `obs` [O, n]: the nodes observed infected or recovered
    in at least one of them, ascending; every node if there is none.  A tensor is reduced where it lies; the ids come back as
    a host array."""
    if isinstance(obs, torch.Tensor):
        seen = (obs >= 1).any(0).cpu().numpy()
    else:
        seen = (np.asarray(obs).astype(np.int64) >= 1).any(0)
    cand = np.flatnonzero(seen)
    return cand if cand.size else np.arange(seen.shape[0])


def source_scores_batch(graph, obs, gamma, maxTime, candidates=None, floor=1e-30, budget_bytes=1 << 30, device="cuda"):
    """`source_scores` for O snapshots of one graph in one pass of the recurrence: a float64 device tensor [O, C, maxTime], and
    scores[o] equals source_scores(graph, obs[o], gamma, maxTime, candidates=candidates, floor=floor) BIT FOR BIT.  A
    candidate's marginals do not depend on the observation, so the node pass computes the three possible terms of a node once
    and every snapshot selects its own (`gnode_dmp_source_batch_scores_f32`): the rank of the true source over many Monte-Carlo
    realisations (`source_rank_of`), or several hypotheses about one incomplete observation, cost one message passing per
    candidate (per tile of `gnode_dmp_source_batch_tile` snapshots on a graph small enough for the one-workgroup form).

    obs: O >= 1 rows of n whole numbers, 0 / 1 / 2 = observed susceptible / infected / recovered, -1 = not observed: a list of
    lists, an array or a tensor.  An integer device tensor -- what `sir_state_at` returns -- is used where it lies and never
    copied to the host.  candidates: node ids (repeats allowed), shared by the snapshots; by default
    `source_candidates_batch(obs)`.  graph, gamma, floor and maxTime are `source_scores`'.  The candidates go to the library in
    chunks of the largest C whose `gnode_dmp_source_batch_workspace_bytes` for these O snapshots fits `budget_bytes`; a budget
    too small for one candidate raises ValueError.  For host inputs, what is wrong raises ValueError before the library is
    loaded or a graph handle is made."""
    entries = ("gnode_dmp_source_batch_workspace_bytes", "gnode_dmp_source_batch_scores_f32")
    return _scores_of_rows("source_scores_batch", "obs", 2, entries, graph, obs, gamma, maxTime, candidates, floor, budget_bytes, device)


def _scores_of_rows(who, name, top, entries, graph, obs, gamma, maxTime, candidates, floor, budget_bytes, device):
    """`source_scores_batch` and `source_scores_events`: the rows `obs` (called `name`) of codes -1 .. top, checked, and the
    candidates in chunks through the library's `entries` = (workspace query, scoring call), which share one signature."""
    G = graph if isinstance(graph, DmpGraph) else DmpGraph(graph)
    n, T = G.N, int(maxTime)
    if T < 2:
        raise ValueError(f"{who}: maxTime must be >= 2 (got {maxTime})")
    floor = float(floor)
    if not 0.0 < floor <= 1.0 or not 0.0 < float(np.float32(floor)) <= 1.0:        # (a NaN fails it; so does a float32 zero)
        raise ValueError(f"{who}: floor must be in (0, 1] as a float32 (got {floor})")
    o = _source_obs_rows(obs, n, who, name, top)
    cand = source_candidates_batch(o) if candidates is None else _source_ints("candidates", candidates, who=who)
    if cand.size < 1:
        raise ValueError(f"{who}: need at least one candidate")
    if cand.min() < 0 or cand.max() >= n:
        raise ValueError(f"{who}: candidate {int(cand[(cand < 0) | (cand >= n)][0])} is not in [0, {n})")
    g = _batch_numbers("gamma", gamma, [(), (n,)], who)
    budget, O, C = int(budget_bytes), int(o.shape[0]), int(cand.size)
    lib, handle = _lib.load(), G.graph.handle
    need_bytes, scores_f32 = (getattr(lib, e) for e in entries)
    need = lambda c: int(need_bytes(handle, c, O, T))               # noqa: E731  (grows with c, or is constant)
    chunk = _largest_chunk(need, C, budget, who)
    up = lambda a, dt: None if a.size == 0 else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)      # noqa: E731
    wd, gd, cd = up(G.data, np.float32), up(np.broadcast_to(g, (n,)), np.float32), up(cand, np.int32)
    od = o.to(torch.int8).contiguous() if isinstance(o, torch.Tensor) else up(o, np.int8)
    scores = torch.empty((O, C, T), dtype=torch.float64, device=cd.device)
    ws = torch.empty(need(chunk), dtype=torch.uint8, device=cd.device)
    for at in range(0, C, chunk):
        c = min(chunk, C - at)
        _lib.check(scores_f32(handle, _lib.ptr(wd), _lib.ptr(gd), _lib.ptr(cd[at:at + c]), c, _lib.ptr(od), O, floor, T,
                              _lib.ptr(scores[0, at:at + c]), C * T, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    return scores


def source_candidates_events(rows):
    """The candidates `source_scores_events` takes by default for the rows [R, n]: the nodes with a code >= 1 -- infected,
    recovered, or seen to become either -- in at least one row, ascending; every node if there is none."""
    return source_candidates_batch(rows)


def source_scores_events(graph, rows, gamma, maxTime, candidates=None, floor=1e-30, budget_bytes=1 << 30, device="cuda"):
    """`source_scores_batch` for evidence that is an EVENT as well as a state: a float64 device tensor [R, C, maxTime],
    scores[r, c, t] = the log-likelihood of row r at model step t under DMP started from candidate c alone.  A row holds one code
    per node: -1 not observed, 0 / 1 / 2 susceptible / infected / recovered at step t (as `source_scores_batch`), 3 = became
    infected AT step t (`t_inf == t` of `sir_trajectories`), with probability Ps(t-1) - Ps(t), 4 = recovered AT step t
    (`t_rec == t`), with probability Pr(t) - Pr(t-1); before the start everybody is susceptible, Ps(-1) = 1 and Pr(-1) = 0, so at
    t = 0 a code 3 is certain at the candidate and at the floor elsewhere.  The differences are float32, of `dmp_batch`'s
    marginals bit for bit, clamped to [floor, 1] before the float64 logarithm; they are taken in the node pass that holds both
    steps in registers (`gnode_dmp_source_events_scores_f32`) and no marginal reaches global memory.  A row of codes -1 .. 2
    equals `source_scores_batch`'s row bit for bit, and no row depends on the others or on the chunking.

    rows: R >= 1 rows of n whole numbers in -1 .. 4; an integer device tensor is used where it lies.  candidates: by default
    `source_candidates_events(rows)`.  Everything else is `source_scores_batch`'s, the chunking by
    `gnode_dmp_source_events_workspace_bytes` included.  `timed_observations` packs records taken at different times into such
    rows and `source_scores_timed` adds their shifted tables."""
    entries = ("gnode_dmp_source_events_workspace_bytes", "gnode_dmp_source_events_scores_f32")
    return _scores_of_rows("source_scores_events", "rows", 4, entries, graph, rows, gamma, maxTime, candidates, floor, budget_bytes,
                           device)


def _whole_number(who, name, value, lowest):
    """`value` as an int >= lowest; ValueError otherwise."""
    try:
        whole = int(value)
        ok = whole == value and whole >= lowest
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"{who}: {name} must be a whole number >= {lowest} (got {value!r})")
    return whole


def source_scores_schedule(weight_adj, rows, gamma, maxTime, observed_at=None, candidates=None, scale=None, floor=1e-30,
                           budget_bytes=1 << 30, device="cuda"):
    """`source_scores_events` when the rates change over time -- who started this outbreak, given that contacts were cut on day
    10 and the snapshot was taken on day 17?  A float64 device tensor [R, C, maxTime].

    weight_adj, scale and gamma may each be a `gnode.ode_nn.RateSchedule`, joined exactly as `dmp_batch` joins them (one
    sparsity pattern, a weight times its scale and every gamma in [0, 1], the schedules need not change at the same steps);
    a scale is None or one number per phase, gamma a number or per-node values: the tables are shared by the candidates.  rows
    holds codes -1 .. 4 as in `source_scores_events`; a row of codes -1 .. 2 is a snapshot, so this call serves what
    `source_scores` and `source_scores_batch` serve under constant rates.  The schedules are stated in CALENDAR steps:
      observed_at=None   the schedule counts from the outbreak's start: scores[r, c, t] = the log-likelihood of row r, t steps
                         after c was seeded at calendar step 0, where step t of the run is governed by the schedule's step t.
      observed_at=D      the rows were taken at calendar step D, a whole number >= maxTime - 1.  "c started tau steps before"
                         places the run's step t at calendar step D - tau + t, so every tau is a run of its own: the samples
                         are (c, shift D - tau) for tau = 0 .. maxTime - 1, and scores[r, c, tau] = that run's value at t = tau.
                         The schedules are read up to calendar step D (`phase_of_step(D + 1)`: a `steps=` schedule shorter
                         than that raises ValueError).  This costs maxTime full-length runs per candidate, of which about
                         half the steps are never read: the run of tau continues past calendar step D, under step D's
                         tables, and is read at t = tau only.
    A sample's marginals are `dmp_batch`'s under `rate_schedule(values, steps=` the phase row from its shift on `)` from the
    seed list [c], bit for bit, and the sums are `source_scores_events`' (`gnode_dmp_source_events_scores_schedule_f32`): with
    schedules that change nothing the table is that call's bit for bit, and no entry depends on the other samples or on the
    chunking.  The samples -- C, or C * maxTime -- go to the library in chunks of the largest count whose
    `gnode_dmp_source_events_schedule_workspace_bytes` fits `budget_bytes`.  candidates, floor: `source_scores_events`'.  The
    result feeds `rank_sources` (a row of it) and `source_rank_of`.  What is wrong raises ValueError before the library is
    loaded or a graph handle is made."""
    who = "source_scores_schedule"
    T = _whole_number(who, "maxTime", maxTime, 2)
    floor = float(floor)
    if not 0.0 < floor <= 1.0 or not 0.0 < float(np.float32(floor)) <= 1.0:        # (a NaN fails it; so does a float32 zero)
        raise ValueError(f"{who}: floor must be in (0, 1] as a float32 (got {floor})")
    D = None if observed_at is None else _whole_number(who, "observed_at", observed_at, T - 1)
    G, datas = _schedule_graph(who, weight_adj)
    n = G.N
    o = _source_obs_rows(rows, n, who, "rows", 4)
    cand = source_candidates_events(o) if candidates is None else _source_ints("candidates", candidates, who=who)
    if cand.size < 1:
        raise ValueError(f"{who}: need at least one candidate")
    if cand.min() < 0 or cand.max() >= n:
        raise ValueError(f"{who}: candidate {int(cand[(cand < 0) | (cand >= n)][0])} is not in [0, {n})")
    phase, w, gam = _schedule_tables(who, G, datas, weight_adj, scale, gamma, T if D is None else D + 1)
    R, C, P = int(o.shape[0]), int(cand.size), int(gam.shape[0])
    if D is None:
        ids, shifts = cand.astype(np.int32), np.zeros(C, dtype=np.int32)
    else:                                                           # sample c * T + tau = (c, D - tau)
        ids, shifts = np.repeat(cand, T).astype(np.int32), np.tile(D - np.arange(T), C).astype(np.int32)
        # every run is full-length, so the run of tau goes on to calendar step D - tau + T - 1 > D: steps that no entry of the
        # result reads (entry tau stops at t = tau, calendar step D).  They are run under step D's phase.
        phase = np.ascontiguousarray(np.concatenate([phase, np.full(T - 1, phase[-1], dtype=np.int32)]))
    L = int(phase.shape[0])
    N, budget = int(ids.size), int(budget_bytes)
    lib, handle = _lib.load(), G.graph.handle
    need = lambda c: int(lib.gnode_dmp_source_events_schedule_workspace_bytes(handle, c, R, T, L))       # noqa: E731
    chunk = _largest_chunk(need, N, budget, who)
    up = lambda a, dt: None if a.size == 0 else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)      # noqa: E731
    wd, gd, cd = up(w, np.float32), up(gam, np.float32), up(ids, np.int32)
    od = o.to(torch.int8).contiguous() if isinstance(o, torch.Tensor) else up(o, np.int8)
    table = torch.empty((R, N, T), dtype=torch.float64, device=cd.device)
    ws = torch.empty(need(chunk), dtype=torch.uint8, device=cd.device)
    for at in range(0, N, chunk):
        c = min(chunk, N - at)
        part = np.ascontiguousarray(shifts[at:at + c])
        _lib.check(lib.gnode_dmp_source_events_scores_schedule_f32(
            handle, _lib.ptr(wd), _lib.ptr(gd), _lib.host_ptr(phase), P, L, _lib.ptr(cd[at:at + c]), _lib.host_ptr(part), c, _lib.ptr(od), R,
            floor, T, _lib.ptr(table[0, at:at + c]), N * T, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    if D is None:
        return table
    return torch.diagonal(table.view(R, C, T, T), dim1=2, dim2=3).contiguous()       # [r, c, tau] = sample (c, tau) at t = tau


class TimedObservations:
    """Records (node, offset, kind) packed into rows for `source_scores_events`, by `timed_observations`: `rows` int8 [R, n]
    (-1 where a row has no record of a node), `row_offsets` int64 [R], the offset every record of a row shares (<= 0, steps
    relative to "now"), and `row_events` int64 [R], how many records of the row have a kind other than 0.  Host arrays."""

    def __init__(self, rows, row_offsets, row_events):
        self.rows, self.row_offsets, self.row_events = rows, row_offsets, row_events
        self.n = int(rows.shape[1])


def timed_observations(n, nodes, offsets, kinds):
    """Pack time-stamped records into a `TimedObservations`.  Record i says that node nodes[i] was seen offsets[i] <= 0 steps
    from "now" in kind kinds[i]: 0 / 1 / 2 susceptible / infected / recovered then, 3 became infected at that step, 4 recovered
    at that step (`source_scores_events`' codes).  A row holds records of ONE offset and at most one per node, so that the
    kernel sums a row in its fixed order and the rows are added in a fixed order after it: the distinct offsets are packed in
    descending order, 0 first, and within an offset a node's j-th record, in input order, goes to that offset's j-th row -- an
    offset has as many rows as its most-observed node has records.  What is wrong raises ValueError."""
    who = "timed_observations"
    try:
        size = int(n)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: n must be a whole number >= 1 (got {n!r})") from None
    if size != n or size < 1:
        raise ValueError(f"{who}: n must be a whole number >= 1 (got {n!r})")
    node, off, kind = (_source_ints(name, v, who=who) for name, v in (("nodes", nodes), ("offsets", offsets), ("kinds", kinds)))
    if not node.shape == off.shape == kind.shape or node.size < 1:
        raise ValueError(f"{who}: nodes, offsets and kinds must be three sequences of one length >= 1, got {node.size}, {off.size}, {kind.size}")
    if node.min() < 0 or node.max() >= size:
        raise ValueError(f"{who}: node {int(node[(node < 0) | (node >= size)][0])} is not in [0, {size})")
    if off.max() > 0:
        raise ValueError(f"{who}: offset {int(off.max())} is after now: offsets are <= 0")
    if kind.min() < 0 or kind.max() > 4:
        raise ValueError(f"{who}: kind {int(kind[(kind < 0) | (kind > 4)][0])} is not in 0 .. 4")
    rows, row_offsets = [], []
    for d in sorted(set(off.tolist()), reverse=True):
        first, seen = len(rows), {}
        for k, code in zip(node[off == d].tolist(), kind[off == d].tolist()):
            j = seen.get(k, 0)
            seen[k] = j + 1
            if first + j == len(rows):
                rows.append(np.full(size, -1, dtype=np.int8))
                row_offsets.append(d)
            rows[first + j][k] = code
    rows = np.stack(rows)
    return TimedObservations(rows, np.asarray(row_offsets, dtype=np.int64), (rows >= 1).sum(1).astype(np.int64))


def sum_timed_rows(table, row_offsets, row_events, floor):
    """The shift-and-add of `source_scores_timed` on a `source_scores_events` table [R, C, T] (a tensor, summed where it lies,
    or an array): float64 [C, T], out[c, t] = the sum over r, taken with explicit adds in ascending r from 0.0, of
    table[r, c, t + row_offsets[r]] where t + row_offsets[r] >= 0 and of row_events[r] * log(float64(float32(floor))) where it is
    not -- before the outbreak everybody is susceptible with probability 1 and every other kind is at the floor (exactly 0.0
    for a row without such a record)."""
    s = table if isinstance(table, torch.Tensor) else torch.from_numpy(np.asarray(table, dtype=np.float64))
    off, events = _source_ints("row_offsets", row_offsets, who="sum_timed_rows"), _source_ints("row_events", row_events, who="sum_timed_rows")
    if s.dim() != 3 or s.dtype != torch.float64 or off.shape[0] != s.shape[0] or events.shape[0] != s.shape[0] or (off.size and off.max() > 0):
        raise ValueError(f"sum_timed_rows: need a float64 table [R, C, T] with R offsets <= 0 and R counts, got {tuple(s.shape)}, "
                         f"{off.shape[0]}, {events.shape[0]}")
    R, C, T = s.shape
    before = float(np.log(np.float64(np.float32(floor))))
    out = torch.zeros((C, T), dtype=torch.float64, device=s.device)
    for r in range(R):
        back = min(-int(off[r]), T)                                   # the row's model step is t - back
        term = torch.full((C, T), int(events[r]) * before if events[r] else 0.0, dtype=torch.float64, device=s.device)
        term[:, back:] = s[r, :, :T - back]
        out = out + term
    return out


def source_scores_timed(graph, observations, gamma, maxTime, candidates=None, floor=1e-30, budget_bytes=1 << 30, device="cuda"):
    """Which node started the outbreak, from records taken at DIFFERENT times -- onset or detection times at a few sensors,
    recovery dates, tests on different days, twice for one person?  A float64 device tensor [C, maxTime]: scores[c, t] = the
    log-likelihood of all records of `observations` (a `TimedObservations`) when "now" is t steps after candidate c was seeded.
    It is `sum_timed_rows` of `source_scores_events(graph, observations.rows, ...)`: row r, whose records lie row_offsets[r]
    steps before now, is read at model step t + row_offsets[r], and where that is before the outbreak a record of kind 0 is
    certain and every other at the floor.  candidates: by default the nodes with a record of a kind other than 0, ascending
    (`source_candidates_events(observations.rows)`).  The other arguments are `source_scores_events`'; `rank_sources` reads the
    result."""
    who = "source_scores_timed"
    if not isinstance(observations, TimedObservations):
        raise ValueError(f"{who}: observations must be what timed_observations returns, got {type(observations).__name__}")
    table = source_scores_events(graph, observations.rows, gamma, maxTime, candidates, floor, budget_bytes, device)
    return sum_timed_rows(table, observations.row_offsets, observations.row_events, floor)


_EVENT_SOURCES = ("onset", "removal", "state")


def observations_from_events(t_inf, t_rec, now, sensors, what=("onset",)):
    """What the nodes `sensors` of ONE trajectory report at step `now`, as the (nodes, offsets, kinds) of `timed_observations`.
    t_inf, t_rec: the trajectory's event steps [n] (a row of `sir_trajectories`' tensors, or arrays; -1 = never).  what: any of
    "onset" -- kind 3 at offset t_inf - now for a sensor with 0 <= t_inf <= now, kind 0 (still susceptible) at offset 0 for
    any other; "removal" -- kind 4 at offset t_rec - now for a sensor with 0 <= t_rec <= now, nothing for one not yet
    recovered; "state" -- `sir_state_at`'s code at offset 0.  The records come in the order of `what`, then of `sensors`.  Runs on
    the host."""
    who = "observations_from_events"
    ti, tr, ids = (_source_ints(name, v, who=who) for name, v in (("t_inf", t_inf), ("t_rec", t_rec), ("sensors", sensors)))
    if ti.shape != tr.shape or ti.size < 1:
        raise ValueError(f"{who}: t_inf and t_rec must be two 1-D rows of one length >= 1, got {ti.size} and {tr.size}")
    if ids.size and (ids.min() < 0 or ids.max() >= ti.size):
        raise ValueError(f"{who}: sensor {int(ids[(ids < 0) | (ids >= ti.size)][0])} is not in [0, {ti.size})")
    t = _source_ints("now", [now], who=who)[0]
    if t < 0:
        raise ValueError(f"{who}: now must be >= 0 (got {now})")
    what = (what,) if isinstance(what, str) else tuple(what)
    if not what or any(w not in _EVENT_SOURCES for w in what):
        raise ValueError(f"{who}: what must name some of {_EVENT_SOURCES}, got {what!r}")
    nodes, offsets, kinds = [], [], []
    for w in what:
        for k in ids.tolist():
            infected, recovered = 0 <= ti[k] <= t, 0 <= tr[k] <= t
            if w == "onset":
                record = (int(ti[k] - t), 3) if infected else (0, 0)
            elif w == "removal":
                record = (int(tr[k] - t), 4) if recovered else None
            else:
                record = (0, int(infected) + int(recovered))
            if record is not None:
                nodes.append(k); offsets.append(record[0]); kinds.append(record[1])
    return nodes, offsets, kinds


def source_rank_of(scores, candidates, truth):
    """How well was each snapshot's true source found?  For a `source_scores_batch` table [O, C, T] and the true source truth[o]
    of every snapshot, an int64 tensor [O]: the number of candidates whose best score over time is STRICTLY greater than that
    of the candidate equal to truth[o] -- 0 means the true source is ranked first, and a tie costs nothing.  A candidate id
    that is repeated takes its first position; a truth[o] that is not among the candidates raises ValueError.  scores may be a
    tensor, and is then ranked where it lies, or an array."""
    s = scores if isinstance(scores, torch.Tensor) else torch.from_numpy(np.asarray(scores, dtype=np.float64))
    cand = _source_ints("candidates", candidates, who="source_rank_of")
    true = _source_ints("truth", truth, who="source_rank_of")
    if s.dim() != 3 or s.shape[0] != true.shape[0] or s.shape[1] != cand.shape[0] or s.shape[2] < 1:
        raise ValueError(f"source_rank_of: scores {tuple(s.shape)} is not [O = {true.shape[0]}, C = {cand.shape[0]}, T >= 1]")
    first = {}
    for i, k in enumerate(cand.tolist()):
        first.setdefault(k, i)
    missing = [k for k in true.tolist() if k not in first]
    if missing:
        raise ValueError(f"source_rank_of: the true source {missing[0]} is not among the candidates")
    best = s.detach().max(2).values                                  # [O, C]
    at = torch.tensor([first[k] for k in true.tolist()], dtype=torch.int64, device=s.device)
    return (best > best.gather(1, at.view(-1, 1))).sum(1)


def rank_sources(scores, candidates):
    """The candidates of a `source_scores` table, most likely first: a list of (candidate, t, score) sorted by the candidate's
    best score over time, descending (ties keep the table's order), with the t at which it is attained."""
    s = scores.detach().cpu().numpy() if isinstance(scores, torch.Tensor) else np.asarray(scores, dtype=np.float64)
    cand = np.asarray(candidates).astype(np.int64).reshape(-1)
    if s.ndim != 2 or s.shape[0] != cand.shape[0] or s.shape[1] < 1:
        raise ValueError(f"rank_sources: scores {tuple(s.shape)} is not one row per candidate ({cand.shape[0]})")
    best_t = s.argmax(1)
    best = s[np.arange(s.shape[0]), best_t]
    order = np.argsort(-best, kind="stable")
    return [(int(cand[i]), int(best_t[i]), float(best[i])) for i in order]


_OUTBREAK_ACTIONS = {"seed": 0, "immunise": 1}


class _Outbreak:
    """The checked, host-side half of an `outbreak_sizes` call -- graph, gamma, value, horizon -- and, from `device_tables` on,
    the device tables and the library: made once, then `sizes` serves any start, candidate list and action on them (the rounds
    of the greedy helpers).  Everything in __init__ raises ValueError and touches neither the library nor a graph handle."""

    def __init__(self, who, graph, gamma, maxTime, value, budget_bytes):
        self.who = who
        self.G = graph if isinstance(graph, DmpGraph) else DmpGraph(graph)
        self.n, self.T = self.G.N, int(maxTime)
        if self.T < 2:
            raise ValueError(f"{who}: maxTime must be >= 2 (got {maxTime})")
        self.gamma = None if gamma is None else _batch_numbers("gamma", gamma, [(), (self.n,)], who)      # (None: the caller's tables)
        self.value = None if value is None else _batch_numbers("value", value, [(self.n,)], who)
        self.budget = int(budget_bytes)
        self.tables = None

    def start(self, start):
        """`start` -- None, a seed list or an `InitialState` -- as an InitialState of this graph's size."""
        from .ode_nn import InitialState
        if isinstance(start, InitialState):
            if start.n != self.n:
                raise ValueError(f"{self.who}: InitialState of {start.n} nodes given for a graph of {self.n}")
            return start
        seeds = [] if start is None else _source_ints("start", start, who=self.who)
        return InitialState.from_sets(self.n, seeds)                 # (a seed outside the graph: ValueError)

    def candidates(self, candidates, lowest):
        """The candidate ids, every node by default, as an int64 array with at least one entry, each in [lowest, n)."""
        cand = np.arange(self.n, dtype=np.int64) if candidates is None else _source_ints("candidates", candidates, who=self.who)
        if cand.size < 1:
            raise ValueError(f"{self.who}: need at least one candidate")
        if cand.min() < lowest or cand.max() >= self.n:
            raise ValueError(f"{self.who}: candidate {int(cand[(cand < lowest) | (cand >= self.n)][0])} is not in [{lowest}, {self.n})")
        return cand

    def device_tables(self, device):
        if self.tables is None:
            lib, handle = _lib.load(), self.G.graph.handle
            up = lambda a: None if a is None or a.size == 0 else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)  # noqa: E731
            self.tables = (lib, handle, up(self.G.data), up(np.broadcast_to(self.gamma, (self.n,))), up(self.value))
        return self.tables

    def sizes(self, start, cand, action, device):
        """float64 device tensor [C, maxTime, 3]: the candidates in chunks of the largest C whose workspace fits the budget."""
        lib, handle, wd, gd, vd = self.device_tables(device)
        T = self.T
        need = lambda c: int(lib.gnode_dmp_outbreak_workspace_bytes(handle, c, T))       # noqa: E731  (grows with c, or is constant)
        chunk = _largest_chunk(need, int(cand.size), self.budget, self.who)
        y0 = torch.from_numpy(start.p.astype(np.float32)).to(device)
        cd = torch.from_numpy(cand.astype(np.int32)).to(device)
        out = torch.empty((cand.size, T, 3), dtype=torch.float64, device=cd.device)
        ws = torch.empty(need(chunk), dtype=torch.uint8, device=cd.device)
        for at in range(0, cand.size, chunk):
            c = min(chunk, cand.size - at)
            _lib.check(lib.gnode_dmp_outbreak_sizes_f32(handle, _lib.ptr(wd), _lib.ptr(gd), _lib.ptr(y0), _lib.ptr(cd[at:at + c]), c,
                                                        _OUTBREAK_ACTIONS[action], _lib.ptr(vd), T, _lib.ptr(out[at:at + c]), _lib.ptr(ws),
                                                        ws.numel(), _lib.stream_ptr()))
        return out


def _outbreak_action(who, action, start):
    if action not in _OUTBREAK_ACTIONS:
        raise ValueError(f"{who}: action must be one of {sorted(_OUTBREAK_ACTIONS)}, got {action!r}")
    if action == "immunise" and not (start.p[:, 1] > 0.0).any():
        raise ValueError(f"{who}: nothing to immunise against: the start holds no infected mass")


def outbreak_sizes(graph, gamma, maxTime, candidates=None, action="seed", start=None, value=None, budget_bytes=1 << 30, device="cuda"):
    """Whom to immunise, or where to seed?  For every candidate node c, the expected size of each compartment over time under
    DMP when c alone is changed in the outbreak `start`: a float64 device tensor [C, maxTime, 3],
    sizes[c, t, j] = sum over the nodes k of value[k] * P^k_j(t),  j = 0 / 1 / 2 for S / I / R,  t = 0 .. maxTime - 1 (row 0 is the
    start itself).  action="seed": c starts infected, (0, 1, 0); action="immunise": c starts removed, (0, 0, 1).  The
    probabilities are `dmp_batch`'s float32 marginals from that start, bit for bit, but they never reach global memory: the sums
    are taken in float64, in a fixed order, in the node pass that holds them in registers (`gnode_dmp_outbreak_sizes_f32`), so a
    candidate's rows do not depend on the other candidates or on the chunking.  `infections(sizes)` reads the number ever
    infected off the table.

    graph: one matrix, as `DMP_SIR` takes, or a `DmpGraph` made from one; its `data` gives the weights.  gamma: a number or
    per-node values [n], finite and >= 0.  start: an `InitialState`, a seed list, or None -- everybody susceptible; "immunise"
    needs some infected mass in it.  candidates: node ids (repeats allowed), every node by default; -1 means "no change" and
    gives the row of `start` as it is.  value: None -- every node counts 1 -- or n finite numbers >= 0, taken as float32.  The
    candidates go to the library in chunks of the largest C whose `gnode_dmp_outbreak_workspace_bytes` fits `budget_bytes` (the
    one-workgroup form needs no room per candidate: one chunk); a budget too small for one candidate raises ValueError.  What
    is wrong raises ValueError before the library is loaded or a graph handle is made."""
    who = "outbreak_sizes"
    plan = _Outbreak(who, graph, gamma, maxTime, value, budget_bytes)
    base = plan.start(start)
    _outbreak_action(who, action, base)
    return plan.sizes(base, plan.candidates(candidates, -1), action, device)


def outbreak_sizes_schedule(weight_adj, gamma, maxTime, candidates=None, action="seed", start=None, value=None, scale=None, shifts=None,
                            budget_bytes=1 << 30, device="cuda"):
    """`outbreak_sizes` when the rates change over time -- whom do we immunise now, given the reopening planned for day 25?  A
    float64 device tensor [C, maxTime, 3], sizes[c, t, j] as `outbreak_sizes` defines it.

    weight_adj, scale and gamma may each be a `gnode.ode_nn.RateSchedule`, joined as `source_scores_schedule` joins them; the
    tables are shared by the candidates.  shifts: None -- the schedule counts from the start of every run -- or one whole
    number >= 0 per candidate: step t of candidate c's run is governed by the schedule's step shifts[c] + t, a run that starts
    shifts[c] steps into the calendar.  candidates=[-1] * K with shifts=range(K) gives the outbreak as it is, started at each
    of K steps: what each step of delay costs.  The schedules are read up to step max(shifts) + maxTime - 1
    (`phase_of_step(max(shifts) + maxTime)`; a `steps=` schedule shorter than that raises ValueError).  A sample's marginals
    are `dmp_batch`'s under the phase row from its shift on, bit for bit, and the sums are `outbreak_sizes`'
    (`gnode_dmp_outbreak_sizes_schedule_f32`): with schedules that change nothing the table is that call's bit for bit.
    candidates, action, start, value, budget_bytes (by `gnode_dmp_outbreak_schedule_workspace_bytes`): `outbreak_sizes`';
    `infections(sizes)` reads the result as before.  What is wrong raises ValueError before the library is loaded or a graph
    handle is made."""
    who = "outbreak_sizes_schedule"
    T = _whole_number(who, "maxTime", maxTime, 2)
    G, datas = _schedule_graph(who, weight_adj)
    plan = _Outbreak(who, G, None, T, value, budget_bytes)
    base = plan.start(start)
    _outbreak_action(who, action, base)
    cand = plan.candidates(candidates, -1)
    C = int(cand.size)
    if shifts is None:
        sh = np.zeros(C, dtype=np.int64)
    else:
        sh = _source_ints("shifts", shifts, C, who=who)
        if sh.min() < 0:
            raise ValueError(f"{who}: shift {int(sh.min())} is negative: a run starts at calendar step 0 or later")
    L = int(sh.max()) + T
    phase, w, gam = _schedule_tables(who, G, datas, weight_adj, scale, gamma, L)
    P, sh = int(gam.shape[0]), sh.astype(np.int32)
    lib, handle = _lib.load(), G.graph.handle
    need = lambda c: int(lib.gnode_dmp_outbreak_schedule_workspace_bytes(handle, c, T, L))       # noqa: E731
    chunk = _largest_chunk(need, C, plan.budget, who)
    up = lambda a, dt: None if a is None or a.size == 0 else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)      # noqa: E731
    wd, gd, vd = up(w, np.float32), up(gam, np.float32), up(plan.value, np.float32)
    y0, cd = up(base.p, np.float32), up(cand, np.int32)
    out = torch.empty((C, T, 3), dtype=torch.float64, device=cd.device)
    ws = torch.empty(need(chunk), dtype=torch.uint8, device=cd.device)
    for at in range(0, C, chunk):
        c = min(chunk, C - at)
        part = np.ascontiguousarray(sh[at:at + c])
        _lib.check(lib.gnode_dmp_outbreak_sizes_schedule_f32(
            handle, _lib.ptr(wd), _lib.ptr(gd), _lib.host_ptr(phase), P, L, _lib.ptr(y0), _lib.ptr(cd[at:at + c]), _lib.host_ptr(part), c,
            _OUTBREAK_ACTIONS[action], _lib.ptr(vd), T, _lib.ptr(out[at:at + c]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    return out


def infections(sizes):
    """The expected value-weighted number ever infected by the horizon for every candidate of an `outbreak_sizes` table: the
    float64 [C] quantity sizes[:, -1, 1] + sizes[:, -1, 2] - sizes[:, 0, 2] -- infected or removed at the end, less those removed
    at the start (the immunised among them), who never were infected.  A tensor gives a tensor, anything else a numpy array."""
    s = sizes if isinstance(sizes, torch.Tensor) else np.asarray(sizes, dtype=np.float64)
    if s.ndim != 3 or s.shape[1] < 1 or s.shape[2] != 3:
        raise ValueError(f"infections: sizes must have the shape [C, maxTime, 3], got {tuple(s.shape)}")
    if isinstance(s, torch.Tensor):
        s = s.double()
    return s[:, -1, 1] + s[:, -1, 2] - s[:, 0, 2]


def _greedy(who, action, graph, start, gamma, maxTime, k, candidates, value, budget_bytes, device):
    """k rounds of one `outbreak_sizes` call each over the pool -- the distinct candidates that are not yet chosen and not
    already fully infected or removed in the start -- on one `_Outbreak`: the round's best node (lowest id among equals) gets
    the action's triple in the start of the next round."""
    from .ode_nn import initial_state
    plan = _Outbreak(who, graph, gamma, maxTime, value, budget_bytes)
    cur = plan.start(start)
    _outbreak_action(who, action, cur)
    pool = np.unique(plan.candidates(candidates, 0))                 # ascending: argmin / argmax take the lowest id among equals
    pool = pool[cur.p[pool, 0] > 0.0]
    try:
        rounds = int(k)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: k must be a whole number (got {k!r})") from None
    if rounds != k or rounds < 1 or rounds > pool.size:
        raise ValueError(f"{who}: k must be a whole number in [1, {pool.size}], the candidates still susceptible (got {k!r})")
    triple = (0.0, 1.0, 0.0) if action == "seed" else (0.0, 0.0, 1.0)
    chosen = []
    for _ in range(rounds):
        inf = infections(plan.sizes(cur, pool, action, device)).cpu().numpy()
        i = int(inf.argmax() if action == "seed" else inf.argmin())
        p = cur.p.copy()
        p[pool[i]] = triple
        cur = initial_state(p)
        chosen.append((int(pool[i]), float(inf[i])))
        pool = np.delete(pool, i)
    return chosen


def greedy_immunisation(graph, start, gamma, maxTime, k, candidates=None, value=None, budget_bytes=1 << 30, device="cuda"):
    """k nodes to immunise against the outbreak `start` (an `InitialState` or a seed list, with some infected mass), chosen
    greedily: each round makes one `outbreak_sizes(..., action="immunise")` call over the candidates not yet chosen and not
    already fully infected or removed, and the node with the fewest `infections` (the lowest id among equals) joins the
    start's removed.  Returns [(node, infections_after), ...] in the order chosen.  The graph handle and the device tables are
    made once for all rounds.  candidates: node ids in [0, n), every node by default; k must not exceed what is left of them.
    What is wrong raises ValueError before the library is loaded or a graph handle is made."""
    return _greedy("greedy_immunisation", "immunise", graph, start, gamma, maxTime, k, candidates, value, budget_bytes, device)


def greedy_seeds(graph, gamma, maxTime, k, start=None, candidates=None, value=None, budget_bytes=1 << 30, device="cuda"):
    """k nodes whose seeding spreads furthest, chosen greedily on top of `start` (None: everybody susceptible): `greedy_immunisation`
    with action="seed" and the node with the MOST `infections` each round, which then starts infected in the next."""
    return _greedy("greedy_seeds", "seed", graph, start, gamma, maxTime, k, candidates, value, budget_bytes, device)
