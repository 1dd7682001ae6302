"""GPU: the gradients of the DMP marginals under a rate schedule (gnode_dmp_batch_schedule_backward_f32,
gnode.dmp.dmp_marginals_schedule) against autograd through the float64 restatement of the scheduled recurrence
(tests/dmp_schedule_grad_model.py), at the bar of tests/test_gpu_baselines.py: errors are max |a - b| / max |b| per gradient
tensor ([P, nnz], [P, n], [n, 3]), `yard` is the float32 restatement's own distance to float64, and the kernels have to meet
gpu_err <= max(4 yard, 1e-6) with yard <= 2.5e-5.  The mistake this bar is there for -- theta_{t+1}'s weight gradient given to
step t's table -- lies at 1e-1 .. 6e-1 on every case with an edge pass (tests/test_dmp_schedule_grad_model.py).

Cases: tests/dmp_grad_model.py's graphs with W = [w, 0.25 w, 0.6 w], G = [gam, min(2.5 gam, 1), 0.5 gam] and the phases spread
over the steps, phase 0 again at the last one; T = 2 (no edge pass), T = 3 (one), every step its own phase (P = T - 1), nnz = 0,
a phase no step names (exact zeros), a graph on each side of gnode_dmp_batch_backward_lds_bytes = 160 KiB, found by asking the
library.  One phase is gnode_dmp_batch_backward_f32 BIT FOR BIT on a graph of each form; a sample inside a batch is its own
B = 1 call bit for bit.  Every workspace is filled with 0xFF first, so nothing is read before it is written.

Measured on an MI355X (gpu_err against yard, for the gradients of W / gamma / init; the bar is max(4 yard, 1e-6)):
    case                            gpu_err W / gamma / init          yard W / gamma / init
    er300 mixed T = 2               1.3e-7 / 5.3e-8 / 9.8e-8          1.3e-7 / 5.3e-8 / 9.8e-8
    er300 mixed T = 3               1.8e-7 / 1.9e-7 / 1.4e-7          1.8e-7 / 1.9e-7 / 1.4e-7
    er300 mixed T = 8               1.7e-7 / 2.0e-7 / 1.5e-7          1.7e-7 / 2.2e-7 / 1.2e-7
    er300 seeds T = 8               1.9e-7 / 1.8e-7 / 2.8e-7          1.9e-7 / 1.8e-7 / 1.9e-7
    er34 w0 / gamma01 mixed T = 12  2.5e-7 / 1.5e-7 / 1.1e-7          2.5e-7 / 1.4e-7 / 1.3e-7
    isolated 513/40 mixed T = 7     8.4e-8 / 8.4e-8 / 1.1e-7          8.8e-8 / 8.4e-8 / 1.1e-7
    nnz = 0, five nodes, T = 6      -      / 8.9e-8 / 7.6e-8          -      / 8.9e-8 / 7.6e-8
    hub mixed T = 10                1.8e-7 / 1.1e-7 / 3.1e-7          1.8e-7 / 1.1e-7 / 5.0e-7
    hub seeds T = 10                1.9e-7 / 3.6e-7 / 6.3e-7          2.5e-7 / 1.5e-7 / 7.1e-7
    er300 T = 3, P = 2              1.7e-7 / 9.7e-8 / 1.1e-7          1.6e-7 / 9.7e-8 / 1.1e-7
    er300 T = 8, P = 7              1.9e-7 / 2.3e-7 / 1.3e-7          1.9e-7 / 2.3e-7 / 1.5e-7
    last fit [0], [1]               5.7e-7 / 6.3e-7 / 2.9e-7, 2.9e-7 / 5.5e-7 / 3.4e-7    the same figures to two digits
    first unfit [0], [1]            5.7e-7 / 5.6e-7 / 3.0e-7, 3.2e-7 / 7.2e-7 / 2.4e-7    5.6e-7 / 5.6e-7 / 3.0e-7, 3.2e-7 / 7.2e-7 / 2.3e-7
    shared tables, B = 3            1.7e-7 / 2.2e-7 / 1.4e-7          1.2e-7 / 2.2e-7 / 1.8e-7
    one scale per phase, d/ds       1.4e-7                            8.4e-8
(Every gpu_err is below its bar; the largest ratio to it is hub seeds' gamma, 3.6e-7 against 1e-6.)  The fit ends at
(0.9999966, 0.3000008, 0.7000107), loss 7.36 -> 9.2e-10: 1.1e-5 from the truth, where the CPU models end.
"""
import functools

import numpy as np
import pytest

import dmp_grad_model as M
import dmp_schedule_grad_model as S
from baseline_cases import assert_schedule_parents, er as _er, gammas as _gammas, rel as _rel, schedule_entry, weights as _weights
from sir_cases import dev, state as _state  # noqa: F401

pytestmark = pytest.mark.gpu

LDS_WORKGROUP = 160 * 1024          # what a gfx950 workgroup may declare
ARG, WORKSPACE = -1, -3             # GNODE_ERR_ARG, GNODE_ERR_WORKSPACE of include/gnode.h
N_FORMS, T_FORMS = 120, 6
PHASE_FORMS = np.asarray([0, 2, 2, 1, 1, 0], dtype=np.int32)       # T_FORMS steps: a change into the last step, phase 0 revisited


class Entry:
    """The scheduled forward and backward C entries (and the constant backward) on one graph, device tensors of the caller's making.
    Tables are host arrays: W [P, nnz] (stride 0) or [B, P, nnz], Gam [P, n] or [B, P, n]."""

    def __init__(self, rp, ci, dev):
        from gnode import _lib
        from gnode.graph import DeviceGraph
        self.lib, self.dev, self.g = _lib.load(), dev, DeviceGraph(rp, ci)
        self.n, self.nnz = len(rp) - 1, len(ci)

    def up(self, a):
        import torch
        a = np.array(a, dtype=np.float32)                            # (a copy: the cases' arrays are read-only)
        return None if a.size == 0 else torch.from_numpy(a).to(self.dev)           # (no edge, no table)

    def lds_bytes(self):
        return int(self.lib.gnode_dmp_batch_backward_lds_bytes(self.g.handle))

    def strides(self, W, Gam):
        P = np.shape(Gam)[-2]
        return P, (P * self.nnz if np.ndim(W) == 3 else 0), (P * self.n if np.ndim(Gam) == 3 else 0)

    def forward(self, W, Gam, phase, init, T):
        import torch
        from gnode import _lib
        B = init.shape[0]
        P, ws_, gs_ = self.strides(W, Gam)
        out = torch.empty((B, T, self.n, 3), dtype=torch.float32, device=self.dev)
        ws = torch.full((int(self.lib.gnode_dmp_batch_schedule_workspace_bytes(self.g.handle, B, T)),), 0xFF, dtype=torch.uint8, device=self.dev)
        wd, gd, yd = self.up(W), self.up(Gam), self.up(init)         # (held: a pointer does not keep its tensor alive)
        ph = np.ascontiguousarray(phase, dtype=np.int32)
        rc = self.lib.gnode_dmp_batch_schedule_f32(self.g.handle, _lib.ptr(wd), ws_, _lib.ptr(gd), gs_, _lib.host_ptr(ph), P, _lib.ptr(yd), B, T,
                                                   _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        assert rc == 0, self.lib.gnode_last_error().decode()
        return out

    def need(self, B, T):
        return int(self.lib.gnode_dmp_batch_schedule_backward_workspace_bytes(self.g.handle, B, T))

    def grads(self, B, P, want=(True, True, True), fill=None):
        import torch
        shapes = ((B, P, self.nnz), (B, P, self.n), (B, self.n, 3))
        return [torch.full(s, np.nan if fill is None else fill, dtype=torch.float32, device=self.dev) if on and np.prod(s) else None
                for s, on in zip(shapes, want)]

    def call(self, w, w_stride, gam, gamma_stride, phase, P, init, B, T, out, G, grads, ws, nbytes=None):
        from gnode import _lib
        ph = None if phase is None else _lib.host_ptr(phase)
        return self.lib.gnode_dmp_batch_schedule_backward_f32(self.g.handle, _lib.ptr(w), w_stride, _lib.ptr(gam), gamma_stride, ph, P, _lib.ptr(init),
                                                              B, T, _lib.ptr(out), _lib.ptr(G), *(_lib.ptr(g) for g in grads), _lib.ptr(ws),
                                                              ws.numel() if nbytes is None else nbytes, _lib.stream_ptr())

    def backward(self, W, Gam, phase, init, T, out, G, want=(True, True, True)):
        """(grad_W [B, P, nnz], grad_G [B, P, n], grad_init [B, n, 3]) as host arrays; None where not wanted (or empty)"""
        import torch
        B = init.shape[0]
        P, ws_, gs_ = self.strides(W, Gam)
        ws = torch.full((self.need(B, T),), 0xFF, dtype=torch.uint8, device=self.dev)       # NaNs, should anything read before it writes
        grads, Gd = self.grads(B, P, want), self.up(G)
        wd, gd, yd = self.up(W), self.up(Gam), self.up(init)
        rc = self.call(wd, ws_, gd, gs_, np.ascontiguousarray(phase, dtype=np.int32), P, yd, B, T, out, Gd, grads, ws)
        assert rc == 0, self.lib.gnode_last_error().decode()
        return [None if g is None else g.cpu().numpy() for g in grads]

    def constant(self, w, gam, init, T, G):
        """gnode_dmp_batch_f32 and gnode_dmp_batch_backward_f32 of host arrays w [nnz] or [B, nnz], gam [n] or [B, n]: (out, grads)"""
        import torch
        from gnode import _lib
        B = init.shape[0]
        wd, gd, yd, Gd = self.up(w), self.up(gam), self.up(init), self.up(G)
        ws_, gs_ = self.nnz if np.ndim(w) == 2 else 0, self.n if np.ndim(gam) == 2 else 0
        out = torch.empty((B, T, self.n, 3), dtype=torch.float32, device=self.dev)
        ws = torch.empty(self.lib.gnode_dmp_batch_workspace_bytes(self.g.handle, B), dtype=torch.uint8, device=self.dev)
        rc = self.lib.gnode_dmp_batch_f32(self.g.handle, _lib.ptr(wd), ws_, _lib.ptr(gd), gs_, _lib.ptr(yd), B, T, _lib.ptr(out), _lib.ptr(ws),
                                          ws.numel(), _lib.stream_ptr())
        assert rc == 0, self.lib.gnode_last_error().decode()
        ws = torch.full((int(self.lib.gnode_dmp_batch_backward_workspace_bytes(self.g.handle, B, T)),), 0xFF, dtype=torch.uint8, device=self.dev)
        shapes = ((B, self.nnz), (B, self.n), (B, self.n, 3))
        grads = [torch.full(s, np.nan, dtype=torch.float32, device=self.dev) if np.prod(s) else None for s in shapes]
        rc = self.lib.gnode_dmp_batch_backward_f32(self.g.handle, _lib.ptr(wd), ws_, _lib.ptr(gd), gs_, _lib.ptr(yd), B, T, _lib.ptr(out),
                                                   _lib.ptr(Gd), *(_lib.ptr(g) for g in grads), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        assert rc == 0, self.lib.gnode_last_error().decode()
        return out, [None if g is None else g.cpu().numpy() for g in grads]


def _meets_the_bar(tag, got, lo, hi):
    """got: the kernels' (grad_W, grad_G, grad_init) of one sample; lo, hi: the float32 and float64 models' (out, grads...)"""
    for key, g, a32, a64 in zip(("W", "gamma", "init"), got, lo[1:], hi[1:]):
        if a64.size == 0:
            assert g is None or g.size == 0
            continue
        assert g.shape == a64.shape and np.isfinite(g).all()
        if not a64.any():
            assert not g.any() and not a32.any(), f"{tag} d/d{key}"
            continue
        yard, gpu_err = _rel(a32, a64), _rel(g, a64)
        print(f"dmp schedule grad {tag} d/d{key}: gpu_err={gpu_err:.3e} yard={yard:.3e}")
        assert yard <= 2.5e-5
        assert gpu_err <= max(4 * yard, 1e-6), f"{tag} d/d{key}"
        for p in range(a64.shape[0]) if key != "init" else ():      # a table without a gradient has none here either
            assert a64[p].any() or not g[p].any(), f"{tag} d/d{key}: phase {p} must be exact zeros"


# ------------------------------------------------------------------ the float64 model's bar
CASES = [("er300_T2", "mixed"), ("er300_T3", "mixed"), ("er300_T8", "mixed"), ("er300_T8", "seeds"), ("er34", "mixed"),
         ("isolated", "mixed"), ("nnz0", "mixed"), ("hub", "mixed"), ("hub", "seeds")]


@pytest.mark.parametrize("name,start", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_gradients_meet_the_models_bar(name, start, dev):
    c = S.case(name, start)
    e = Entry(c["rp"], c["ci"], dev)
    assert (e.lds_bytes() > LDS_WORKGROUP) == (name == "hub")                   # the hub is the general form's case
    init, T = c["init"][None], c["T"]
    out = e.forward(c["W"], c["Gam"], c["phase"], init, T)
    lo, hi = S.model(name, start, "float32"), S.model(name, start, "float64")
    assert _rel(out[0].cpu().numpy(), hi[0]) <= 1e-5
    got = e.backward(c["W"], c["Gam"], c["phase"], init, T, out, c["G"][None])
    _meets_the_bar(f"{name}/{start}", [None if g is None else g[0] for g in got], lo, hi)
    if T == 2 and e.nnz:                                            # no edge pass: theta_1's weight alone, phase[1]'s table
        p1 = int(c["phase"][1])
        assert got[0][0, p1].any() and not np.delete(got[0][0], p1, axis=0).any()
        assert got[1][0, p1].any() and not np.delete(got[1][0], p1, axis=0).any()
    again = e.backward(c["W"], c["Gam"], c["phase"], init, T, out, c["G"][None])
    for a, b in zip(got, again):                                    # two calls, equal bits
        assert (a is None and b is None) or np.array_equal(a, b)


def _factor_tables(w, gam, P):
    """P tables: the weights times 1, 0.85, 0.7, ... and the gammas times 1, 1.1, 1.2, ... capped at 1"""
    W = np.stack([(w * np.float32(1.0 - 0.15 * p)).astype(np.float32) for p in range(P)])
    G = np.stack([np.minimum(gam * np.float32(1.0 + 0.1 * p), np.float32(1.0)).astype(np.float32) for p in range(P)])
    return W, G


@pytest.mark.parametrize("name", ["er300_T3", "er300_T8"])
def test_every_step_its_own_phase(name, dev):
    """P = T - 1, phase[t] = t - 1: each step's adjoint goes to a table of its own, and the last table is only ever a `next` weight
    and a node pass's gamma."""
    c = M.case(name)
    T, P = c["T"], c["T"] - 1
    W, Gam = _factor_tables(c["w"], c["gam"], P)
    phase = np.concatenate([[0], np.arange(P)]).astype(np.int32)
    e = Entry(c["rp"], c["ci"], dev)
    out = e.forward(W, Gam, phase, c["init"][None], T)
    got = e.backward(W, Gam, phase, c["init"][None], T, out, c["G"][None])
    lo, hi = (S.gradients(c["rp"], c["ci"], W, Gam, phase, c["init"], T, c["G"], d) for d in ("float32", "float64"))
    assert all(hi[1][p].any() and hi[2][p].any() for p in range(P))
    _meets_the_bar(f"{name} P={P}", [g[0] for g in got], lo, hi)


# ------------------------------------------------------------------ both forms and the boundary between them
def _w(rp, ci, seed):
    """Weights that are not symmetric in value, sized to the mean degree so that long rows neither die out nor saturate."""
    s = min(1.0, 5.0 * (len(rp) - 1) / max(len(ci), 1))
    return _weights(len(ci), 0.05 * s, 0.4 * s, seed)


@functools.lru_cache(maxsize=None)
def form_graphs():
    """{tag: (rp, ci)} at n = 120: the largest m whose backward still fits one workgroup's LDS, and the next m, which does not.
    The sizes are the library's answers."""
    from gnode import _lib
    from gnode.graph import DeviceGraph

    def at(m):
        rp, ci, _ = _er(N_FORMS, m, 40)
        g = DeviceGraph(rp, ci)                                     # (kept: the handle dies with it)
        return rp, ci, int(_lib.load().gnode_dmp_batch_backward_lds_bytes(g.handle))
    lo, hi = 2000, N_FORMS * (N_FORMS - 1) // 2                     # lo fits, hi does not
    assert at(lo)[2] <= LDS_WORKGROUP < at(hi)[2]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if at(mid)[2] <= LDS_WORKGROUP else (lo, mid)
    g = {"last_fit": at(lo), "first_unfit": at(hi)}
    assert g["last_fit"][2] <= LDS_WORKGROUP < g["first_unfit"][2]
    return {k: v[:2] for k, v in g.items()}


def _entry_graph(form):
    if form == "general":
        return form_graphs()["first_unfit"]
    c = M.case("er300_T8")
    return c["rp"], c["ci"]


def _batch_inputs(rp, ci, B, seed, P=3):
    """B samples: per-sample tables [B, P, ...], starts alternately mixed states and seed lists, and grad_out"""
    n = len(rp) - 1
    tabs = [S.three_tables(_w(rp, ci, seed + b), _gammas(n, seed + 10 + b)) for b in range(B)]
    W, Gam = np.stack([t[0][:P] for t in tabs]), np.stack([t[1][:P] for t in tabs])
    init = np.stack([M.mixed_state(n, seed + 20 + b) if b % 2 == 0 else M.seed_state(n, [b, n - 1 - b]) for b in range(B)])
    return W, Gam, init, np.random.default_rng(seed).standard_normal((B, T_FORMS, n, 3)).astype(np.float32)


@pytest.mark.parametrize("tag", ["last_fit", "first_unfit"])
def test_each_side_of_the_lds_boundary(tag, dev):
    rp, ci = form_graphs()[tag]
    e = Entry(rp, ci, dev)
    assert (e.lds_bytes() <= LDS_WORKGROUP) == (tag == "last_fit")
    B, T = 2, T_FORMS
    W, Gam, init, G = _batch_inputs(rp, ci, B, 50)
    out = e.forward(W, Gam, PHASE_FORMS, init, T)
    got = e.backward(W, Gam, PHASE_FORMS, init, T, out, G)
    for b in range(B):
        lo, hi = (S.gradients(rp, ci, W[b], Gam[b], PHASE_FORMS, init[b], T, G[b], d) for d in ("float32", "float64"))
        assert float((hi[0][0, :, 0] - hi[0][-1, :, 0]).max()) > 0.05          # something spread
        _meets_the_bar(f"{tag}[{b}]", [g[b] for g in got], lo, hi)


@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_one_phase_is_the_constant_call(form, dev):
    """P = 1: the three gradients are gnode_dmp_batch_backward_f32's bit for bit, shared and per-sample tables.  Three phases
    holding equal tables: the constant gradient is spread over the phases, each slot summing its own steps' terms in the
    constant sweep's order; summed over the phases in float64 it is the constant gradient up to the order of at most 2 (T - 1)
    float32 additions per entry, so 2 T float32 eps of the tensor's largest entry is the bound, and the start's gradient, which no
    phase splits, is equal bit for bit."""
    rp, ci = _entry_graph(form)
    e = Entry(rp, ci, dev)
    assert (e.lds_bytes() <= LDS_WORKGROUP) == (form == "one_workgroup")
    B, T = 3, T_FORMS
    W, Gam, init, G = _batch_inputs(rp, ci, B, 100, P=1)
    for w_shared, g_shared in ((False, False), (True, True), (True, False)):
        Wc, Gc = W[0] if w_shared else W, Gam[0] if g_shared else Gam
        out_c, want = e.constant(Wc[..., 0, :], Gc[..., 0, :], init, T, G)
        out = e.forward(Wc, Gc, np.zeros(T, np.int32), init, T)
        assert np.array_equal(out.cpu().numpy(), out_c.cpu().numpy())
        got = e.backward(Wc, Gc, np.zeros(T, np.int32), init, T, out, G)
        for key, a, b in zip(("W", "gamma", "init"), got, want):
            assert np.isfinite(b).all() and np.abs(b).max() > 0
            assert np.array_equal(a.reshape(b.shape), b), f"{form}, shared {w_shared} {g_shared}: d/d{key} with one phase is not the constant call's"
    W3, G3 = np.repeat(W, 3, axis=1), np.repeat(Gam, 3, axis=1)
    out_c, want = e.constant(W[:, 0], Gam[:, 0], init, T, G)
    out = e.forward(W3, G3, PHASE_FORMS, init, T)
    assert np.array_equal(out.cpu().numpy(), out_c.cpu().numpy())
    got = e.backward(W3, G3, PHASE_FORMS, init, T, out, G)
    assert np.array_equal(got[2], want[2])
    eps = float(np.finfo(np.float32).eps)
    for key, a, b in zip(("W", "gamma"), got, want):
        total = a.astype(np.float64).sum(1)
        assert np.abs(total - b).max() <= 2 * T * eps * np.abs(b).max(), f"{form}: d/d{key}"


@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_a_sample_of_a_batch_is_its_own_call_and_an_unnamed_phase_is_zero(form, dev):
    """B = 1, 3, 5 with shared (stride 0) and per-sample tables: block b is the B = 1 call of sample b bit for bit, whatever B is,
    and one block per sample comes back where the table is shared.  P = 4 with phase 3 never named: exact zeros there, and the
    other three tables' gradients are the P = 3 call's bits."""
    rp, ci = _entry_graph(form)
    e = Entry(rp, ci, dev)
    T = T_FORMS
    W, GAM, INIT, G = _batch_inputs(rp, ci, 5, 200)
    solo = {}

    def alone(b, w_shared, g_shared):
        key = (0 if w_shared else b, 0 if g_shared else b, b)
        if key not in solo:
            Wb, Gb = W[key[0]], GAM[key[1]]
            out = e.forward(Wb, Gb, PHASE_FORMS, INIT[b:b + 1], T)
            solo[key] = (out, e.backward(Wb, Gb, PHASE_FORMS, INIT[b:b + 1], T, out, G[b:b + 1]))
        return solo[key]
    for B in (5, 3, 1):
        for w_shared, g_shared in ((False, False), (True, False), (False, True), (True, True)):
            Wc, Gc = W[0] if w_shared else W[:B], GAM[0] if g_shared else GAM[:B]
            out = e.forward(Wc, Gc, PHASE_FORMS, INIT[:B], T)
            got = e.backward(Wc, Gc, PHASE_FORMS, INIT[:B], T, out, G[:B])
            assert [g.shape for g in got] == [(B, 3, e.nnz), (B, 3, e.n), (B, e.n, 3)]
            for b in range(B):
                out1, want = alone(b, w_shared, g_shared)
                assert np.array_equal(out[b].cpu().numpy(), out1[0].cpu().numpy())
                for key, a, s in zip(("W", "gamma", "init"), got, want):
                    assert np.isfinite(s).all() and np.abs(s).max() > 0
                    assert np.array_equal(a[b], s[0]), f"{form} B={B} shared W {w_shared} gamma {g_shared}: d/d{key} of sample {b}"
    B = 2
    W4 = np.concatenate([W[:B], np.full((B, 1, e.nnz), 0.5, np.float32)], axis=1)
    G4 = np.concatenate([GAM[:B], np.full((B, 1, e.n), 0.5, np.float32)], axis=1)
    out = e.forward(W4, G4, PHASE_FORMS, INIT[:B], T)
    got4 = e.backward(W4, G4, PHASE_FORMS, INIT[:B], T, out, G[:B])
    got3 = e.backward(W[:B], GAM[:B], PHASE_FORMS, INIT[:B], T, out, G[:B])
    assert not got4[0][:, 3].any() and not got4[1][:, 3].any()
    assert np.array_equal(got4[0][:, :3], got3[0]) and np.array_equal(got4[1][:, :3], got3[1]) and np.array_equal(got4[2], got3[2])


@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_each_gradient_pointer_may_be_null(form, dev):
    rp, ci = _entry_graph(form)
    e = Entry(rp, ci, dev)
    W, Gam, init, G = _batch_inputs(rp, ci, 2, 300)
    out = e.forward(W, Gam, PHASE_FORMS, init, T_FORMS)
    full = e.backward(W, Gam, PHASE_FORMS, init, T_FORMS, out, G)
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, True), (True, False, False)):
        got = e.backward(W, Gam, PHASE_FORMS, init, T_FORMS, out, G, want)
        for i in range(3):
            assert (got[i] is None) if not want[i] else np.array_equal(got[i], full[i]), (want, i)


@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_refusals_write_nothing_and_a_good_call_is_served(form, dev):
    import torch
    rp, ci = _entry_graph(form)
    e = Entry(rp, ci, dev)
    B, T, P, n, nnz = 2, T_FORMS, 3, len(rp) - 1, len(ci)
    W, Gam, init, G = _batch_inputs(rp, ci, B, 400)
    out, Gd = e.forward(W, Gam, PHASE_FORMS, init, T), e.up(G)
    full = e.backward(W, Gam, PHASE_FORMS, init, T, out, G)
    need = e.need(B, T)
    assert need > 2 * B * (T - 1) * nnz * 4 and e.need(0, T) == 0 and e.need(B, 1) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    grads = e.grads(B, P, fill=-7.0)
    wd, gd, yd, ph = e.up(W), e.up(Gam), e.up(init), PHASE_FORMS
    sw, sg = P * nnz, P * n
    call = lambda **k: e.call(**{**dict(w=wd, w_stride=sw, gam=gd, gamma_stride=sg, phase=ph, P=P, init=yd, B=B, T=T, out=out, G=Gd,     # noqa: E731
                                        grads=grads, ws=ws), **k})
    said = lambda: e.lib.gnode_last_error().decode()                # noqa: E731
    assert call(nbytes=need - 1) == WORKSPACE
    assert call(B=0) == ARG and call(T=1) == ARG and call(P=0) == ARG
    assert call(P=2, w_stride=2 * nnz, gamma_stride=2 * n) == ARG and "phase[" in said()             # a phase of 2 with P = 2
    bad = ph.copy(); bad[T - 1] = -1
    assert call(phase=bad) == ARG
    assert call(grads=[None, None, None]) == ARG
    for ws_, gs_ in ((nnz, sg), (sw - 1, sg), (sw, n), (sw, sg + 1), (-sw, sg), (1, sg)):
        assert call(w_stride=ws_, gamma_stride=gs_) == ARG, (ws_, gs_)
    for missing in ("w", "gam", "init", "out", "G", "ws", "phase"):
        assert call(**{missing: None}, nbytes=need) == ARG, missing
    for value in (float("nan"), 1.5, -0.25):                        # a rate that is no probability: sample, phase and position named
        x = W.copy(); x[1, 2, nnz - 1] = value
        assert call(w=e.up(x)) == ARG and "sample 1" in said() and "phase 2" in said() and f"weights[{nnz - 1}]" in said()
        x = Gam[0].copy(); x[1, 3] = value
        assert call(gam=e.up(x), gamma_stride=0) == ARG and "sample 0" in said() and "phase 1" in said() and "gamma[3]" in said()
    torch.cuda.synchronize()
    assert all(bool((g == -7.0).all()) for g in grads)
    free = ph.copy(); free[0] = 99                                  # entry 0 is never read
    assert call(phase=free) == 0, said()
    for g, f in zip(grads, full):
        assert np.array_equal(g.cpu().numpy(), f)


# ------------------------------------------------------------------ the parent's bits
PARENT_CASES = [(g, t) for g in ("last_fit", "first_unfit") for t in ("per_sample", "shared", "P4")] + [("er300_T2", "P2"), ("nnz0", "P3")]


def parent_entries(name, tables, dev):
    """[(key, entry)] of tests/golden/dmp_schedule_parent.json for one call: the three gradients of the graph on each side of the
    LDS boundary with test_each_side_of_the_lds_boundary's inputs -- per-sample tables, shared ones (sample 0's), and P = 4 where
    no step names phase 3 --, of er300 at T = 2 with two phases (no edge pass) and of the five nodes without an edge.  The block
    of a phase that no step names is exact zeros."""
    if name in ("last_fit", "first_unfit"):
        rp, ci = form_graphs()[name]
        T, phase = T_FORMS, PHASE_FORMS
        W, Gam, init, G = _batch_inputs(rp, ci, 2, 50)
        if tables == "shared":
            W, Gam = W[0], Gam[0]
        elif tables == "P4":
            W = np.concatenate([W, np.full((2, 1, len(ci)), 0.5, np.float32)], axis=1)
            Gam = np.concatenate([Gam, np.full((2, 1, len(rp) - 1), 0.5, np.float32)], axis=1)
    else:
        c = S.case(name)
        rp, ci, T, phase, P = c["rp"], c["ci"], c["T"], c["phase"], int(tables[1:])
        W, Gam, init, G = c["W"][:P], c["Gam"][:P], c["init"][None], c["G"][None]
    e = Entry(rp, ci, dev)
    got = e.backward(W, Gam, phase, init, T, e.forward(W, Gam, phase, init, T), G)
    for p in set(range(np.shape(Gam)[-2])) - set(int(p) for p in phase[1:T]):
        assert all(g is None or not g[:, p].any() for g in got[:2]), (name, tables, p)
    return [(f"backward/{name}/{tables}", schedule_entry(got, e.need(init.shape[0], T), e.lds_bytes() <= LDS_WORKGROUP))]


@pytest.mark.parametrize("name,tables", PARENT_CASES)
def test_gradients_are_the_parents_bits(name, tables, dev):
    """tests/golden/dmp_schedule_parent.json: what the library of commit 8bd479b returned on an MI355X, when the scheduled
    reverse sweep had kernels and a host side of its own."""
    assert_schedule_parents(parent_entries(name, tables, dev))


# ------------------------------------------------------------------ the Python function
def _tensors(dev, W, Gam, init, requires=(True, True, True)):
    import torch
    return [torch.from_numpy(np.array(a, dtype=np.float32)).to(dev).requires_grad_(r) for a, r in zip((W, Gam, init), requires)]


def _graph(rp, ci):
    import scipy.sparse as sp
    from gnode.dmp import DmpGraph
    n = len(rp) - 1
    return DmpGraph(sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n)))


def test_forward_is_dmp_batch_with_the_same_schedule_bit_for_bit(dev):
    import scipy.sparse as sp
    import torch
    from gnode.dmp import dmp_batch, dmp_marginals_schedule
    from gnode.ode_nn import rate_schedule
    for name in ("er300_T8", "hub", "nnz0"):
        c = S.case(name)
        n, B, T, phase = len(c["rp"]) - 1, 3, c["T"], c["phase"]
        mats = [sp.csr_matrix((w.astype(np.float64), c["ci"], c["rp"]), shape=(n, n)) for w in c["W"]]
        init = np.stack([M.mixed_state(n, 500 + b) for b in range(B)])
        Gam = np.stack([S.three_tables(c["w"], _gammas(n, 510 + b))[1] for b in range(B)])              # [B, 3, n]
        want = dmp_batch(rate_schedule(mats, steps=phase), [_state(p) for p in init], rate_schedule([Gam[:, p] for p in range(3)], steps=phase), T)
        W, g, y0 = _tensors(dev, c["W"], Gam, init, (False, False, False))
        got = dmp_marginals_schedule(_graph(c["rp"], c["ci"]), W, g, y0, T, phase)
        assert not got.requires_grad and torch.equal(got, want), name
        by_schedule = dmp_marginals_schedule(_graph(c["rp"], c["ci"]), W, g, y0, T, rate_schedule(["a", "b", "c"], steps=phase))
        assert torch.equal(by_schedule, want), name


@pytest.mark.parametrize("requires", [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (False, True, True)])
def test_backward_fills_the_inputs_that_require_it(requires, dev):
    """.backward() of (out * G).sum() through dmp_marginals_schedule: .grad of exactly the inputs that require one, the C entry's."""
    from gnode.dmp import dmp_marginals_schedule
    c = M.case("er300_T8")
    e = Entry(c["rp"], c["ci"], dev)
    W, Gam, init, _ = _batch_inputs(c["rp"], c["ci"], 3, 600)
    G = np.random.default_rng(601).standard_normal((3, c["T"], e.n, 3)).astype(np.float32)
    phase = S.spread_phases(c["T"])
    ts = _tensors(dev, W, Gam, init, requires)
    out = dmp_marginals_schedule(_graph(c["rp"], c["ci"]), *ts, c["T"], phase)
    assert out.requires_grad
    (out * e.up(G)).sum().backward()
    want = e.backward(W, Gam, phase, init, c["T"], out.detach(), G)
    for t, r, f in zip(ts, requires, want):
        assert (t.grad is not None) == r
        if r:
            assert t.grad.shape == t.shape and np.array_equal(t.grad.cpu().numpy(), f)


def test_backward_reads_the_saved_tensors_autograd_hands_back(dev):
    """Under saved-tensor hooks (save_on_cpu) backward receives new allocations, and the forward's are free to be reused: the
    gradients of both functions are the plain call's bits, with the freed memory overwritten in between.  The tables are
    products made for the call, so nothing else holds them."""
    import torch
    from gnode.dmp import dmp_marginals, dmp_marginals_schedule
    c = M.case("er300_T8")
    e = Entry(c["rp"], c["ci"], dev)
    W, Gam, init, _ = _batch_inputs(c["rp"], c["ci"], 3, 650)
    G = e.up(np.random.default_rng(651).standard_normal((3, c["T"], e.n, 3)).astype(np.float32))
    phase, graph = S.spread_phases(c["T"]), _graph(c["rp"], c["ci"])
    calls = {"schedule": lambda ts: dmp_marginals_schedule(graph, ts[0] * 0.5, ts[1] * 0.5, ts[2], c["T"], phase),
             "constant": lambda ts: dmp_marginals(graph, ts[0][:, 0] * 0.5, ts[1][:, 0] * 0.5, ts[2], c["T"])}
    for name, call in calls.items():
        plain = _tensors(dev, W, Gam, init)
        (call(plain) * G).sum().backward()
        hooked = _tensors(dev, W, Gam, init)
        with torch.autograd.graph.save_on_cpu():
            out = call(hooked)
        junk = [torch.full_like(t, 0.5) for t in hooked for _ in range(4)]         # lands where the forward's tables lay
        (out * G).sum().backward()
        for a, b in zip(plain, hooked):
            assert torch.isfinite(b.grad).all() and b.grad.abs().max() > 0 and torch.equal(a.grad, b.grad), name
        del junk


def test_shared_tables_get_the_sum_over_the_samples(dev):
    """W [P, nnz] and gamma [P, n] shared by B samples: .grad is the sum of the per-sample blocks, held to the model's bar (the
    model: the sum of the B samples' gradients, each by autograd)."""
    import torch
    from gnode.dmp import dmp_marginals_schedule
    c = S.case("er300_T8")
    n, nnz, B, T = len(c["rp"]) - 1, len(c["ci"]), 3, c["T"]
    init = np.stack([M.mixed_state(n, 700), M.seed_state(n, [5, 250]), M.mixed_state(n, 702)])
    G = M.grad_out_of(T, n, B)
    W, gam, y0 = _tensors(dev, c["W"], c["Gam"], init)
    out = dmp_marginals_schedule(_graph(c["rp"], c["ci"]), W, gam, y0, T, c["phase"])
    (out * torch.from_numpy(G).to(dev)).sum().backward()
    assert W.grad.shape == (3, nnz) and gam.grad.shape == (3, n) and y0.grad.shape == (B, n, 3)
    per = {d: [S.gradients(c["rp"], c["ci"], c["W"], c["Gam"], c["phase"], init[b], T, G[b], d) for b in range(B)] for d in ("float32", "float64")}
    lo, hi = ([None, sum(p[1] for p in per[d]), sum(p[2] for p in per[d]), np.stack([p[3] for p in per[d]])] for d in ("float32", "float64"))
    _meets_the_bar("shared tables", [t.grad.cpu().numpy() for t in (W, gam, y0)], lo, hi)


def _scale_model(c, base, gam, s, phase, init, T, G, dtype):
    """d sum(G * out) / ds for weights = base[None, :] * s[:, None], by autograd through the model"""
    import torch
    dt = getattr(torch, dtype)
    src, rev = (torch.from_numpy(a) for a in M.tables(c["rp"], c["ci"]))
    sv = torch.tensor(np.asarray(s, np.float64), dtype=dt, requires_grad=True)
    W = torch.tensor(np.asarray(base, np.float64), dtype=dt)[None, :] * sv[:, None]
    out = S.forward(src, rev, len(c["rp"]) - 1, W, torch.tensor(np.asarray(gam, np.float64), dtype=dt), phase,
                    torch.tensor(np.asarray(init, np.float64), dtype=dt), T)
    (out * torch.tensor(np.asarray(G, np.float64), dtype=dt)).sum().backward()
    return sv.grad.numpy()


def test_one_scale_per_phase_gets_its_gradient_through_torch(dev):
    """weights = base * s[:, None] written in torch: autograd carries the table's gradient to s; held to the float64 model's bar"""
    import torch
    from gnode.dmp import dmp_marginals_schedule
    c = S.case("er300_T8")
    T, phase, s0 = c["T"], c["phase"], np.asarray([1.0, 0.25, 0.6], np.float32)
    s = torch.tensor(s0, device=dev, requires_grad=True)
    base = torch.from_numpy(np.array(c["w"])).to(dev)
    gam, y0 = torch.from_numpy(np.array(c["Gam"])).to(dev), torch.from_numpy(np.array(c["init"][None])).to(dev)
    out = dmp_marginals_schedule(_graph(c["rp"], c["ci"]), base[None, :] * s[:, None], gam, y0, T, phase)
    (out[0] * torch.from_numpy(np.array(c["G"])).to(dev)).sum().backward()
    a32, a64 = (_scale_model(c, c["w"], c["Gam"], s0, phase, c["init"], T, c["G"], d) for d in ("float32", "float64"))
    yard, gpu_err = _rel(a32, a64), _rel(s.grad.cpu().numpy(), a64)
    print(f"dmp schedule grad d/ds: gpu_err={gpu_err:.3e} yard={yard:.3e}")
    assert a64.all() and yard <= 2.5e-5
    assert gpu_err <= max(4 * yard, 1e-6)


# ------------------------------------------------------------------ the fit it is for
def test_three_contact_scales_are_recovered_from_the_curves(dev):
    """er34, base weight 0.3 on every contact, gamma 0.2, phases [-, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]; the target is the scheduled
    dmp_batch at the scales (1.0, 0.3, 0.7).  Adam (lr 0.05, 200 steps) on the squared error from (0.6, 0.6, 0.6), clamped to
    [0, 1 / 0.3], must end within 1e-3 of the truth: on the CPU the float32 and the float64 model both end within 1.1e-5, and
    optimiser paths may part in the last bits."""
    import scipy.sparse as sp
    import torch
    from gnode.dmp import dmp_batch, dmp_marginals_schedule
    from gnode.ode_nn import rate_schedule
    c = M.case("er34", "seeds")
    n, nnz, T = len(c["rp"]) - 1, len(c["ci"]), 12
    assert c["T"] == T
    phase = np.asarray([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int32)
    truth = [1.0, 0.3, 0.7]
    A = sp.csr_matrix((np.full(nnz, np.float64(np.float32(0.3))), c["ci"], c["rp"]), shape=(n, n))
    target = dmp_batch(A, [_state(c["init"])], 0.2, T, scale=rate_schedule(truth, steps=phase))
    graph = _graph(c["rp"], c["ci"])
    base = torch.full((nnz,), 0.3, dtype=torch.float32, device=dev)
    gam = torch.full((3, n), 0.2, dtype=torch.float32, device=dev)
    y0 = torch.from_numpy(np.array(c["init"][None])).to(dev)
    s = torch.full((3,), 0.6, dtype=torch.float32, device=dev, requires_grad=True)
    opt = torch.optim.Adam([s], lr=0.05)
    first = None
    for _ in range(200):
        opt.zero_grad()
        loss = ((dmp_marginals_schedule(graph, base[None, :] * s[:, None], gam, y0, T, phase) - target) ** 2).sum()
        first = float(loss.detach()) if first is None else first
        loss.backward()
        opt.step()
        with torch.no_grad():
            s.clamp_(0.0, 1.0 / 0.3)
    got = s.detach().cpu().numpy()
    print(f"dmp schedule fit: s = {got.tolist()}, loss {first:.3e} -> {float(loss.detach()):.3e}")
    assert first > 1.0
    assert np.abs(got - np.asarray(truth)).max() <= 1e-3
