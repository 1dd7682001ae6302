"""GPU: the gradients of the DMP marginals (gnode_dmp_batch_backward_f32, gnode_dmp_backward_f32, gnode.dmp.dmp_marginals)
against autograd through the float64 restatement of the recurrence (tests/dmp_grad_model.py), at the bar of
tests/test_gpu_baselines.py: errors are max |a - b| / max |b| per gradient tensor, `yard` is the float32 restatement's own
distance to float64, and the kernels have to meet gpu_err <= max(4 yard, 1e-6) with yard <= 2.5e-5.

Cases (tests/dmp_grad_model.py): er(300, 900, 7) at T = 2 (no edge pass: the weights' gradient comes from theta_1 alone), T = 3
(one edge pass, both theta_bar buffers) and T = 8; er(34, 78, 3) with a third of the weights 0 and gamma at 0 and 1;
er(513, 40, 6): rows without edges, n no multiple of a block; five nodes without an edge; chung_lu(3001, 40000)
with a row of 1511 edges (the general form, long row sums); and a graph on each side of
gnode_dmp_batch_backward_lds_bytes = 160 KiB, found by asking the library.  A sample inside a batch is held to the solo entry
(always the general form) BIT FOR BIT, which below the 160 KiB is the one-workgroup form against the general one.

Measured on an MI355X (gpu_err against yard, for the gradients of w / gamma / init; the bar is max(4 yard, 1e-6)):
    case                          gpu_err w / gamma / init          yard w / gamma / init
    er300 mixed T = 2             1.4e-7 / 5.3e-8 / 7.2e-8          1.4e-7 / 5.3e-8 / 7.2e-8
    er300 mixed T = 3             3.0e-7 / 6.7e-8 / 1.0e-7          3.0e-7 / 5.4e-8 / 9.3e-8
    er300 mixed T = 8             1.6e-7 / 1.7e-7 / 1.1e-7          1.6e-7 / 1.7e-7 / 1.4e-7
    er300 seeds T = 8             2.2e-7 / 1.1e-7 / 5.4e-7          3.0e-7 / 1.4e-7 / 4.9e-7
    er34 w0 / gamma01 mixed T = 12  1.7e-7 / 1.5e-7 / 1.4e-7        9.6e-8 / 1.5e-7 / 1.4e-7
    isolated 513/40 mixed T = 7   6.1e-8 / 1.1e-7 / 1.5e-7          1.5e-7 / 1.1e-7 / 1.5e-7
    nnz = 0, five nodes, T = 6    -      / 3.6e-8 / 1.2e-7          -      / 3.6e-8 / 1.2e-7
    hub mixed T = 10              1.2e-7 / 1.2e-7 / 3.0e-7          1.2e-7 / 1.2e-7 / 3.9e-7
    hub seeds T = 10              1.4e-7 / 1.1e-7 / 1.1e-6          1.9e-7 / 1.1e-7 / 9.5e-7
    last fit (m = 2908) [0], [1]  5.4e-7 / 2.1e-7 / 1.9e-7, 2.4e-7 / 1.8e-7 / 2.0e-7    6.2e-7 / 2.1e-7 / 1.8e-7, 2.8e-7 / 1.8e-7 / 1.7e-7
    first unfit (m = 2909)        5.6e-7 / 2.1e-7 / 2.2e-7, 3.2e-7 / 3.6e-7 / 2.7e-7    the same figures to three digits
    one entry (7, 150, Pi)        5.9e-7 / 1.5e-7 / 1.5e-7          4.9e-7 / 1.5e-7 / 1.5e-7
    shared tables, B = 3          1.1e-7 / 1.2e-7 / 2.7e-7          9.1e-8 / 1.2e-7 / 2.1e-7
(Every gpu_err is below a third of its bar.)
"""
import functools

import numpy as np
import pytest

import dmp_grad_model as M
from baseline_cases import er as _er, gammas as _gammas, rel as _rel, weights as _weights
from sir_cases import dev  # noqa: F401

pytestmark = pytest.mark.gpu

LDS_WORKGROUP = 160 * 1024          # what a gfx950 workgroup may declare
ARG, WORKSPACE = -1, -3             # GNODE_ERR_ARG, GNODE_ERR_WORKSPACE of include/gnode.h
N_FORMS, T_FORMS = 120, 6


class Entry:
    """The forward and backward C entries on one graph with device tensors of the caller's making."""

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

    def forward(self, w, gam, init, T):
        """out [B, T, n, 3] of host arrays w [nnz] or [B, nnz], gam [n] or [B, n], init [B, n, 3]"""
        import torch
        from gnode import _lib
        B = init.shape[0]
        out = torch.empty((B, T, self.n, 3), dtype=torch.float32, device=self.dev)
        ws = torch.empty(self.lib.gnode_dmp_batch_workspace_bytes(self.g.handle, B), dtype=torch.uint8, device=self.dev)
        wd, gd, yd = self.up(w), self.up(gam), self.up(init)        # (held: a pointer does not keep its tensor alive)
        rc = self.lib.gnode_dmp_batch_f32(self.g.handle, _lib.ptr(wd), self.nnz if np.ndim(w) == 2 else 0, _lib.ptr(gd),
                                          self.n if np.ndim(gam) == 2 else 0, _lib.ptr(yd), B, T, _lib.ptr(out), _lib.ptr(ws),
                                          ws.numel(), _lib.stream_ptr())
        assert rc == 0, self.lib.gnode_last_error().decode()
        return out

    def need(self, B, T):
        return int(self.lib.gnode_dmp_batch_backward_workspace_bytes(self.g.handle, B, T))

    def grads(self, B, want=(True, True, True), fill=None):
        import torch
        shapes = ((B, self.nnz), (B, self.n), (B, self.n, 3))
        return [torch.full(s, np.nan if fill is None else fill, dtype=torch.float32, device=self.dev) if on and np.prod(s) else None
                for s, on in zip(shapes, want)]

    def backward(self, w, gam, init, T, out, G, want=(True, True, True)):
        """(grad_w, grad_gamma, grad_init) of the batch entry as host arrays; None where not wanted (or empty)"""
        import torch
        B = init.shape[0]
        ws = torch.full((self.need(B, T),), 0xFF, dtype=torch.uint8, device=self.dev)       # NaNs, should anything read before it writes
        grads, Gd = self.grads(B, want), self.up(G)
        rc = self.call(w, gam, init, B, T, out, Gd, grads, ws)
        assert rc == 0, self.lib.gnode_last_error().decode()
        return [None if g is None else g.cpu().numpy() for g in grads]

    def call(self, w, gam, init, B, T, out, G, grads, ws, nbytes=None, w_stride=None, gamma_stride=None):
        from gnode import _lib
        w_stride = (self.nnz if np.ndim(w) == 2 else 0) if w_stride is None else w_stride
        gamma_stride = (self.n if np.ndim(gam) == 2 else 0) if gamma_stride is None else gamma_stride
        dv = lambda a: a if a is None or hasattr(a, "is_cuda") else self.up(a)      # noqa: E731
        wd, gd, yd = dv(w), dv(gam), dv(init)                       # (held: a pointer does not keep its tensor alive)
        return self.lib.gnode_dmp_batch_backward_f32(self.g.handle, _lib.ptr(wd), w_stride, _lib.ptr(gd), gamma_stride, _lib.ptr(yd),
                                                     B, T, _lib.ptr(out), _lib.ptr(G), *(_lib.ptr(g) for g in grads), _lib.ptr(ws),
                                                     ws.numel() if nbytes is None else nbytes, _lib.stream_ptr())

    def solo(self, w, gam, init, T, out, G, want=(True, True, True)):
        """gnode_dmp_backward_f32 for one sample: host arrays w [nnz], gam [n], init [n, 3]; out, G device [T, n, 3]"""
        import torch
        from gnode import _lib
        ws = torch.full((int(self.lib.gnode_dmp_backward_workspace_bytes(self.g.handle, T)),), 0xFF, dtype=torch.uint8, device=self.dev)
        grads = self.grads(1, want)
        wd, gd, yd, out, G = self.up(w), self.up(gam), self.up(init), out.contiguous(), G.contiguous()
        rc = self.lib.gnode_dmp_backward_f32(self.g.handle, _lib.ptr(wd), _lib.ptr(gd), _lib.ptr(yd), T,
                                             _lib.ptr(out), _lib.ptr(G), *(_lib.ptr(g) for g in grads), _lib.ptr(ws),
                                             ws.numel(), _lib.stream_ptr())
        assert rc == 0, self.lib.gnode_last_error().decode()
        return [None if g is None else g[0].cpu().numpy() for g in grads]


def _meets_the_bar(tag, got, lo, hi):
    """got: the kernels' (grad_w, grad_gamma, grad_init); lo, hi: the float32 and float64 models' (out, grads...)"""
    for key, g, a32, a64 in zip(("w", "gamma", "init"), got, lo[1:], hi[1:]):
        if a64.size == 0:
            assert g is None or g.size == 0
            continue
        assert np.isfinite(g).all()
        if not a64.any():                                           # (one marginal of step 1 does not depend on gamma at all)
            assert not g.any() and not a32.any(), f"{tag} d/d{key}"
            continue
        yard, gpu_err = _rel(a32, a64), _rel(g, a64)
        print(f"dmp grad {tag} d/d{key}: gpu_err={gpu_err:.3e} yard={yard:.3e}")
        assert yard <= 2.5e-5
        assert gpu_err <= max(4 * yard, 1e-6), f"{tag} d/d{key}"


# ------------------------------------------------------------------ the float64 model's bar, both entries
CASES = [("er300_T2", "mixed"), ("er300_T3", "mixed"), ("er300_T8", "mixed"), ("er300_T8", "seeds"), ("er34", "mixed"),
         ("isolated", "mixed"), ("nnz0", "mixed"), ("hub", "mixed"), ("hub", "seeds")]


@pytest.mark.parametrize("name,start", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_gradients_meet_the_models_bar(name, start, dev):
    c = M.case(name, start)
    e = Entry(c["rp"], c["ci"], dev)
    assert (e.lds_bytes() > LDS_WORKGROUP) == (name == "hub")                   # the hub is the general form's case
    init = c["init"][None]
    out = e.forward(c["w"], c["gam"], init, c["T"])
    lo, hi = M.model(name, start, "float32"), M.model(name, start, "float64")
    assert _rel(out[0].cpu().numpy(), hi[0]) <= 1e-5
    got = e.backward(c["w"], c["gam"], init, c["T"], out, c["G"][None])
    _meets_the_bar(f"{name}/{start}", [None if g is None else g[0] for g in got], lo, hi)
    solo = e.solo(c["w"], c["gam"], c["init"], c["T"], out[0], e.up(c["G"]))
    for key, a, b in zip(("w", "gamma", "init"), got, solo):
        assert (a is None and b is None) or np.array_equal(a[0], b), f"{name}/{start}: d/d{key} of the batch entry is not the solo entry's"


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


@pytest.mark.parametrize("tag", ["last_fit", "first_unfit"])
def test_each_side_of_the_lds_boundary(tag, dev):
    rp, ci = form_graphs()[tag]
    e = Entry(rp, ci, dev)
    assert (e.lds_bytes() <= LDS_WORKGROUP) == (tag == "last_fit")
    B, T, n = 2, T_FORMS, N_FORMS
    w, gam = np.stack([_w(rp, ci, 50 + b) for b in range(B)]), np.stack([_gammas(n, 60 + b) for b in range(B)])
    init = np.stack([M.mixed_state(n, 70), M.seed_state(n, [3, 77])])
    G = M.grad_out_of(T, n, B)
    out = e.forward(w, gam, init, T)
    got = e.backward(w, gam, init, T, out, G)
    for b in range(B):
        lo, hi = (M.gradients(rp, ci, w[b], gam[b], init[b], T, G[b], d) for d in ("float32", "float64"))
        assert float((hi[0][0, :, 0] - hi[0][-1, :, 0]).max()) > 0.05          # something spread
        _meets_the_bar(f"{tag}[{b}]", [g[b] for g in got], lo, hi)
        solo = e.solo(w[b], gam[b], init[b], T, out[b], e.up(G[b]))
        for key, a, s in zip(("w", "gamma", "init"), got, solo):
            assert np.array_equal(a[b], s), f"{tag}: d/d{key} of sample {b} is not the solo entry's"


# ------------------------------------------------------------------ batches, strides, pointers
def _entry_graph(form):
    if form == "general":
        return form_graphs()["first_unfit"]
    c = M.case("er300_T8")
    return c["rp"], c["ci"]


def _batch_inputs(rp, ci, B, seed):
    """B samples: per-sample weights and gammas, starts alternately mixed states and seed lists, and grad_out"""
    n = len(rp) - 1
    w, gam = np.stack([_w(rp, ci, seed + b) for b in range(B)]), np.stack([_gammas(n, seed + 10 + b) for b in range(B)])
    init = np.stack([M.mixed_state(n, seed + 20 + b) if b % 2 == 0 else M.seed_state(n, [b, n - 1 - b]) for b in range(B)])
    return w, gam, init, np.random.default_rng(seed).standard_normal((B, T_FORMS, n, 3)).astype(np.float32)


@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_a_sample_of_a_batch_is_its_solo_sweep(form, dev):
    """B = 1, 3, 5 with shared (stride 0) and per-sample tables: row b is gnode_dmp_backward_f32's output for sample b bit for
    bit, whatever B is, and one row per sample comes back where the table is shared."""
    rp, ci = _entry_graph(form)
    e = Entry(rp, ci, dev)
    assert (e.lds_bytes() <= LDS_WORKGROUP) == (form == "one_workgroup")
    W, GAM, INIT, G = _batch_inputs(rp, ci, 5, 200)
    first = {}
    for B in (5, 3, 1):
        for w_shared, g_shared in ((False, False), (True, False), (False, True), (True, True)):
            w, gam = W[0] if w_shared else W[:B], GAM[0] if g_shared else GAM[:B]
            out = e.forward(w, gam, INIT[:B], T_FORMS)
            got = e.backward(w, gam, INIT[:B], T_FORMS, out, G[:B])
            assert [g.shape for g in got] == [(B, e.nnz), (B, e.n), (B, e.n, 3)]
            for b in range(B):
                solo = e.solo(W[0] if w_shared else W[b], GAM[0] if g_shared else GAM[b], INIT[b], T_FORMS, out[b], e.up(G[b]))
                for key, a, s in zip(("w", "gamma", "init"), got, solo):
                    assert np.isfinite(s).all() and np.abs(s).max() > 0
                    assert np.array_equal(a[b], s), f"{form} B={B} shared w {w_shared} gamma {g_shared}: d/d{key} of sample {b}"
            first.setdefault((w_shared, g_shared), got)
            for a, a5 in zip(got, first[(w_shared, g_shared)]):                 # row 0 of B = 5 is B = 1
                assert np.array_equal(a[0], a5[0])


@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_each_gradient_pointer_may_be_null(form, dev):
    rp, ci = _entry_graph(form)
    e = Entry(rp, ci, dev)
    w, gam, init, G = _batch_inputs(rp, ci, 2, 300)
    out = e.forward(w, gam, init, T_FORMS)
    full = e.backward(w, gam, init, T_FORMS, out, G)
    for missing in range(3):
        want = tuple(i != missing for i in range(3))
        got = e.backward(w, gam, init, T_FORMS, out, G, want)
        for i in range(3):
            assert (got[i] is None) if i == missing else np.array_equal(got[i], full[i]), (missing, i)
    only = e.backward(w, gam, init, T_FORMS, out, G, (False, False, True))
    assert only[0] is None and only[1] is None and np.array_equal(only[2], full[2])


@pytest.mark.parametrize("t,k,col", [(0, 7, 1), (1, 299, 0), (4, 0, 2), (7, 150, 1)])
def test_one_entry_of_grad_out(t, k, col, dev):
    """grad_out zero but for one (t, k, column): the gradient of one marginal, held to the model's bar."""
    c = M.case("er300_T8")
    e = Entry(c["rp"], c["ci"], dev)
    G = np.zeros((c["T"], e.n, 3), dtype=np.float32)
    G[t, k, col] = 1.0
    out = e.forward(c["w"], c["gam"], c["init"][None], c["T"])
    got = e.backward(c["w"], c["gam"], c["init"][None], c["T"], out, G[None])
    lo, hi = (M.gradients(c["rp"], c["ci"], c["w"], c["gam"], c["init"], c["T"], G, d) for d in ("float32", "float64"))
    if t == 0:                                                      # row 0 is the start itself
        want = np.zeros((e.n, 3), dtype=np.float32)
        want[k, col] = 1.0
        assert np.array_equal(got[2][0], want) and not got[0].any() and not got[1].any()
        return
    _meets_the_bar(f"one entry ({t}, {k}, {col})", [g[0] for g in got], lo, hi)


@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_refusals_write_nothing_and_a_good_call_is_served(form, dev):
    import torch
    rp, ci = _entry_graph(form)
    e = Entry(rp, ci, dev)
    B, T = 2, T_FORMS
    w, gam, init, G = _batch_inputs(rp, ci, B, 400)
    out, Gd = e.forward(w, gam, init, T), e.up(G)
    full = e.backward(w, gam, init, T, out, G)
    need = e.need(B, T)
    assert need > 2 * B * (T - 1) * e.nnz * 4 and e.need(0, T) == 0 and e.need(B, 1) == 0
    assert e.lib.gnode_dmp_backward_workspace_bytes(e.g.handle, 1) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    grads = e.grads(B, fill=-7.0)
    wd, gd, yd = e.up(w), e.up(gam), e.up(init)
    assert e.call(wd, gd, yd, B, T, out, Gd, grads, ws, need - 1) == WORKSPACE
    assert e.call(wd, gd, yd, 0, T, out, Gd, grads, ws) == ARG
    assert e.call(wd, gd, yd, B, 1, out, Gd, grads, ws) == ARG
    assert e.call(wd, gd, yd, B, T, out, Gd, [None, None, None], ws) == ARG
    for ws_, gs_ in ((1, e.n), (e.nnz - 1, e.n), (e.nnz, 1), (e.nnz, e.n + 1), (e.n, e.n), (-e.nnz, e.n)):
        assert e.call(wd, gd, yd, B, T, out, Gd, grads, ws, w_stride=ws_, gamma_stride=gs_) == ARG, (ws_, gs_)
    for missing in ("w", "gam", "init", "out", "G", "ws"):
        a = dict(w=wd, gam=gd, init=yd, out=out, G=Gd, ws=ws)
        a[missing] = None
        assert e.call(a["w"], a["gam"], a["init"], B, T, a["out"], a["G"], grads, a["ws"] if a["ws"] is not None else None, need,
                      w_stride=e.nnz, gamma_stride=e.n) == ARG, missing
    k = e.nnz // 2                                                  # one directed entry out of the middle of the CSR
    row = int(np.searchsorted(rp, k, side="right") - 1)
    rp2 = rp.copy(); rp2[row + 1:] -= 1
    e2 = Entry(rp2, np.delete(ci, k), dev)
    ws2 = torch.empty(e2.need(B, T), dtype=torch.uint8, device=dev)
    assert e2.call(np.delete(w, k, axis=1), gd, yd, B, T, out, Gd, [g[:, :e2.nnz].contiguous() if i == 0 else g for i, g in enumerate(grads)],
                   ws2) == ARG
    assert "symmetric" in e2.lib.gnode_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((g == -7.0).all()) for g in grads)
    assert e.call(wd, gd, yd, B, T, out, Gd, grads, ws) == 0, e.lib.gnode_last_error().decode()
    for g, f in zip(grads, full):
        assert np.array_equal(g.cpu().numpy(), f)


# ------------------------------------------------------------------ the Python function
def _tensors(dev, w, gam, init, requires=(True, True, True)):
    import torch
    return [torch.from_numpy(np.array(a, dtype=np.float32)).to(dev).requires_grad_(r) for a, r in zip((w, gam, init), requires)]


def test_dmp_marginals_is_dmp_batch_bit_for_bit(dev):
    import scipy.sparse as sp
    import torch
    from gnode.dmp import DmpGraph, dmp_batch, dmp_marginals
    from sir_cases import state
    for name in ("er300_T8", "hub", "nnz0"):
        c = M.case(name)
        n, B = len(c["rp"]) - 1, 3
        A = sp.csr_matrix((c["w"].astype(np.float64), c["ci"], c["rp"]), shape=(n, n))
        init = np.stack([M.mixed_state(n, 500 + b) for b in range(B)])
        gam = np.stack([_gammas(n, 510 + b) for b in range(B)])
        want = dmp_batch(A, [state(p) for p in init], gam, c["T"])
        w, g, y0 = _tensors(dev, c["w"], gam, init, (False, False, False))
        got = dmp_marginals(DmpGraph(A), w, g, y0, c["T"])
        assert not got.requires_grad and torch.equal(got, want), name
        scale = [1.0, 0.5, 0.8125]
        want = dmp_batch(A, [state(p) for p in init], gam[0], c["T"], scale=scale)
        w = torch.from_numpy((c["w"].astype(np.float64)[None] * np.asarray(scale)[:, None]).astype(np.float32)).to(dev)
        assert torch.equal(dmp_marginals(DmpGraph(A), w, g[0], y0, c["T"]), want), name


@pytest.mark.parametrize("requires", [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (False, True, True)])
def test_backward_fills_the_inputs_that_require_it(requires, dev):
    """.backward() of (out * G).sum() through dmp_marginals: .grad of exactly the inputs that require one, equal to the C entry's."""
    import torch
    from gnode.dmp import DmpGraph, dmp_marginals
    c = M.case("er300_T8")
    e = Entry(c["rp"], c["ci"], dev)
    w, gam, init, G = _batch_inputs(c["rp"], c["ci"], 3, 600)
    G = np.random.default_rng(601).standard_normal((3, c["T"], e.n, 3)).astype(np.float32)
    import scipy.sparse as sp
    graph = DmpGraph(sp.csr_matrix((np.ones(e.nnz), c["ci"], c["rp"]), shape=(e.n, e.n)))
    ts = _tensors(dev, w, gam, init, requires)
    out = dmp_marginals(graph, *ts, c["T"])
    assert out.requires_grad
    (out * e.up(G)).sum().backward()
    want = e.backward(w, gam, init, c["T"], out.detach(), G)
    for t, r, f in zip(ts, requires, want):
        assert (t.grad is not None) == r
        if r:
            assert t.grad.shape == t.shape and np.array_equal(t.grad.cpu().numpy(), f)


def test_shared_tables_get_the_sum_over_the_samples(dev):
    """weights [nnz] and gamma [n] shared by B samples: .grad is the sum of the per-sample rows, held to the model's bar (the
    model: the sum of the B samples' gradients, each by autograd)."""
    import scipy.sparse as sp
    from gnode.dmp import DmpGraph, dmp_marginals
    c = M.case("er300_T8")
    n, nnz, B, T = len(c["rp"]) - 1, len(c["ci"]), 3, c["T"]
    init = np.stack([M.mixed_state(n, 700), M.seed_state(n, [5, 250]), M.mixed_state(n, 702)])
    G = M.grad_out_of(T, n, B)
    graph = DmpGraph(sp.csr_matrix((np.ones(nnz), c["ci"], c["rp"]), shape=(n, n)))
    w, gam, y0 = _tensors(dev, c["w"], c["gam"], init)
    out = dmp_marginals(graph, w, gam, y0, T)
    import torch
    (out * torch.from_numpy(G).to(dev)).sum().backward()
    assert w.grad.shape == (nnz,) and gam.grad.shape == (n,) and y0.grad.shape == (B, n, 3)
    per = {d: [M.gradients(c["rp"], c["ci"], c["w"], c["gam"], init[b], T, G[b], d) for b in range(B)] for d in ("float32", "float64")}
    lo, hi = ([None, sum(p[1] for p in per[d]), sum(p[2] for p in per[d]), np.stack([p[3] for p in per[d]])] for d in ("float32", "float64"))
    _meets_the_bar("shared tables", [t.grad.cpu().numpy() for t in (w, gam, y0)], lo, hi)
