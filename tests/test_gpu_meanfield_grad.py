"""GPU: the differentiable mean-field -- gnode_meanfield_rates_steps_f64, gnode_meanfield_rates_backward_f64 and
gnode.ode_nn.meanfield_marginals -- against the numpy model of tests/meanfield_grad_model.py replaying the call's own recorded
steps.  The bar is MF_GRAD_RTOL = 64 x float64's rounding as measured against np.longdouble on the CPU
(tests/test_meanfield_grad_model.py), relative to each model array's largest entry; every entry of every array is compared.

Cases (meanfield_grad_model.gpu_cases; rtol 1e-8, atol 1e-10, at most 8 output times, B * n never a multiple of 256): one node
without an edge (w and grad_w NULL); n = 257, B = 1; n = 300, B = 3 with per-sample beta and gamma; a star of 260 nodes (a row of
259 entries, 110 steps in one interval); a graph with self-loops; a fifth of the weights 0 (directed contacts); beta and w NULL;
deltaT = 0.5; an output grid with repeated times; n_out = 1.

Measured on an MI355X: in all ten cases every output and every gradient entry equals the float64 model's exactly (distance 0
against the bar of 1.7e-13) -- the kernels add in the model's order and the library is built without contraction."""
import ctypes as C

import numpy as np
import pytest

import meanfield_grad_model as M
from meanfield_grad_model import MF_GRAD_RTOL
from sir_cases import dev  # noqa: F401

pytestmark = pytest.mark.gpu

ARG, WORKSPACE = -1, -3             # GNODE_ERR_ARG, GNODE_ERR_WORKSPACE of include/gnode.h
KEYS = ("init", "beta", "w", "gamma")   # the entry's order of the gradient pointers
CASES = M.gpu_cases()


class Entry:
    """The C entries on one case, with device tensors of this object's making."""

    def __init__(self, case, dev, rp=None, ci=None):
        import torch
        from gnode import _lib
        from gnode.graph import DeviceGraph
        self.lib, self.dev, self.case = _lib.load(), dev, case
        self.g = DeviceGraph(case["rp"] if rp is None else rp, case["ci"] if ci is None else ci)
        self.B, self.n = case["gamma"].shape
        self.nnz, self.rows, self.t_out = self.g.nnz, self.B * self.n, np.ascontiguousarray(case["t_out"], np.float64)
        self.T = len(self.t_out)
        up = lambda a: None if a is None or a.size == 0 else torch.from_numpy(np.array(a, np.float64)).to(dev)      # noqa: E731
        self.d = {k: up(case[k]) for k in ("init", "beta", "w", "gamma")}

    def _fwd_args(self, out, steps, ws):
        from gnode import _lib
        d = self.d
        return (self.g.handle, self.B, _lib.ptr(d["init"]), _lib.ptr(d["beta"]), _lib.ptr(d["w"]), _lib.ptr(d["gamma"]), _lib.host_ptr(self.t_out),
                self.T, M.RTOL, M.ATOL, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), C.byref(steps), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())

    def _out_ws(self):
        import torch
        out = torch.full((3, self.T, self.rows), np.nan, dtype=torch.float64, device=self.dev)
        ws = torch.empty(self.lib.gnode_meanfield_rates_workspace_bytes(self.g.handle, self.B), dtype=torch.uint8, device=self.dev)
        return out, ws

    def plain(self):
        """gnode_meanfield_rates_f64: (out [3 = I, S, R][T][rows], attempted steps)"""
        out, ws = self._out_ws()
        steps = C.c_int64(0)
        rc = self.lib.gnode_meanfield_rates_f64(*self._fwd_args(out, steps, ws))
        assert rc == 0, self.lib.gnode_last_error().decode()
        return out, steps.value

    def steps(self, cap=4096):
        """gnode_meanfield_rates_steps_f64: (out, attempted steps, h [cap] with what lies past the record untouched, n_h, n_acc)"""
        from gnode import _lib
        out, ws = self._out_ws()
        steps, n_h = C.c_int64(0), C.c_int64(-1)
        h, n_acc = np.full(cap + 2, -5.0), np.full(self.T, -9, np.int32)
        rc = self.lib.gnode_meanfield_rates_steps_f64(*self._fwd_args(out, steps, ws), _lib.host_ptr(h), cap, C.byref(n_h), _lib.host_ptr(n_acc))
        assert rc == 0, self.lib.gnode_last_error().decode()
        return out, steps.value, h, n_h.value, n_acc

    def grad_buffers(self, want, fill=np.nan):
        import torch
        shapes = {"init": (self.B, self.n, 3), "beta": (self.B, self.n), "w": (self.B, self.nnz), "gamma": (self.B, self.n)}
        return {k: torch.full(shapes[k], fill, dtype=torch.float64, device=self.dev) if k in want and np.prod(shapes[k]) else None for k in KEYS}

    def need(self, m):
        return int(self.lib.gnode_meanfield_rates_backward_workspace_bytes(self.g.handle, self.B, int(m)))

    def call_backward(self, out, h, n_acc, g, grads, ws, nbytes=None):
        """the status of gnode_meanfield_rates_backward_f64; g: device [3 = I, S, R][T][rows]"""
        from gnode import _lib
        d = self.d
        h, n_acc = np.ascontiguousarray(h, np.float64), np.ascontiguousarray(n_acc, np.int32)
        return self.lib.gnode_meanfield_rates_backward_f64(
            self.g.handle, self.B, _lib.ptr(d["init"]), _lib.ptr(d["beta"]), _lib.ptr(d["w"]), _lib.ptr(d["gamma"]), _lib.host_ptr(self.t_out), self.T,
            _lib.host_ptr(h), len(h), _lib.host_ptr(n_acc), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.ptr(g[0]), _lib.ptr(g[1]),
            _lib.ptr(g[2]), *(_lib.ptr(grads[k]) for k in KEYS), _lib.ptr(ws), ws.numel() if nbytes is None else nbytes, _lib.stream_ptr())

    def backward(self, out, h, n_acc, g, want=KEYS):
        """{key: host array or None}; the workspace is prefilled with NaNs, should anything be read before it is written"""
        import torch
        ws = torch.full((self.need(n_acc.max(initial=0)),), 0xFF, dtype=torch.uint8, device=self.dev)
        grads = self.grad_buffers(want)
        rc = self.call_backward(out, h, n_acc, g, grads, ws)
        assert rc == 0, self.lib.gnode_last_error().decode()
        torch.cuda.synchronize()
        return {k: None if v is None else v.cpu().numpy() for k, v in grads.items()}


@pytest.fixture(scope="module")
def runs(dev):
    """name -> (Entry, out, attempted, h, n_acc, g on the device, gradients, model gradients, model outputs): each case runs once"""
    import torch
    cache = {}

    def get(name):
        if name not in cache:
            c = CASES[name]
            e = Entry(c, dev)
            out, attempted, hbuf, n_h, n_acc = e.steps()
            h = hbuf[:n_h].copy()
            g_host = M.grad_out(c)
            g = torch.from_numpy(np.stack([x.reshape(e.T, e.rows) for x in g_host])).to(dev)
            grads = e.backward(out, h, n_acc, g)
            args = (c["rp"], c["ci"], c["init"], c["beta"], c["gamma"], c["w"], e.T, h, n_acc)
            cache[name] = (e, out, attempted, h, n_acc, g, grads, M.dp5_replay_grad(*args, *g_host), M.dp5_replay(*args))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_steps_entry_is_the_plain_entry(runs, name):
    e, out, attempted, h, n_acc, *_ = runs(name)
    plain, plain_steps = e.plain()
    assert attempted == plain_steps and np.array_equal(out.cpu().numpy().view(np.int64), plain.cpu().numpy().view(np.int64))
    assert n_acc[0] == 0 and (n_acc >= 0).all() and n_acc.sum() == len(h) <= attempted
    assert (h > 0).all()
    same = np.diff(e.t_out) == 0
    assert (n_acc[1:][same] == 0).all() and (n_acc[1:][~same] > 0).all()
    if len(h) > 2:                                                  # a record that does not fit: the count is whole, the tail is dropped
        _, _, hbuf, n_h, n_acc2 = e.steps(cap=2)
        assert n_h == len(h) and np.array_equal(hbuf[:2], h[:2]) and (hbuf[2:] == -5.0).all() and np.array_equal(n_acc2, n_acc)


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_meet_the_model(runs, name):
    e, out, _, h, n_acc, _, grads, model, model_out = runs(name)
    got_out = out.cpu().numpy()
    for c, want in enumerate(model_out):                            # the model's forward on the call's own steps
        err = M.rel_err(got_out[c], want.reshape(e.T, e.rows))
        print(f"meanfield grad {name} out[{c}]: {err:.3e}")
        assert err <= MF_GRAD_RTOL
    for key in KEYS:
        got, want = grads[key], model[key]
        if key not in M.compared_keys(CASES[name]):                 # no edge: nothing reaches the outputs through beta or w
            assert got is None or not got.any()
            assert not want.any()
            continue
        assert got.shape == want.shape and np.isfinite(got).all()
        if e.T == 1 and key != "init":
            assert not got.any() and not want.any()                 # n_out = 1: only the start's gradient is not 0
            continue
        assert np.max(np.abs(want)) > 0, key                        # a case only counts where the model's gradient is not 0
        err = M.rel_err(got, want)
        print(f"meanfield grad {name} d/d{key}: {err:.3e} of {MF_GRAD_RTOL:.3e}")
        assert err <= MF_GRAD_RTOL, key
    if e.T == 1:                                                    # grad_init is grad_out's row 0, transposed
        g_host = M.grad_out(CASES[name])
        assert np.array_equal(grads["init"], np.stack([g_host[1][0], g_host[0][0], g_host[2][0]], axis=-1))


@pytest.mark.parametrize("name", list(CASES))
def test_two_calls_return_the_same_bits(runs, name):
    e, out, _, h, n_acc, g, grads, *_ = runs(name)
    again = e.backward(out, h, n_acc, g)
    for key in KEYS:
        assert (grads[key] is None) == (again[key] is None)
        if grads[key] is not None:
            assert np.array_equal(grads[key].view(np.int64), again[key].view(np.int64)), key


@pytest.mark.parametrize("name", ["n300_B3", "no_beta_no_w"])
def test_a_subset_leaves_the_others_bits(runs, name):
    e, out, _, h, n_acc, g, grads, *_ = runs(name)
    for want in (("init",), ("beta",), ("w",), ("gamma",), ("beta", "w"), ("init", "gamma")):
        part = e.backward(out, h, n_acc, g, want=want)
        for key in KEYS:
            if key in want:
                assert np.array_equal(part[key].view(np.int64), grads[key].view(np.int64)), (want, key)
            else:
                assert part[key] is None


# ------------------------------------------------------------------ the Python face
def _tensors(c, dev, shared_rows=False):
    import torch
    t = lambda a: None if a is None else torch.from_numpy(np.array(a, np.float64)).to(dev).requires_grad_()      # noqa: E731
    beta, gamma = (c["beta"], c["gamma"]) if not shared_rows else (None if c["beta"] is None else c["beta"][0], c["gamma"][0])
    return t(c["init"]), t(beta), t(gamma), t(c["w"])


def _marginals(e, tensors, deltaT=1, maxTime=None):
    from gnode.ode_nn import meanfield_marginals
    init, beta, gamma, w = tensors
    return meanfield_marginals(e.g, init, beta, gamma, w, deltaT=deltaT, maxTime=e.T if maxTime is None else maxTime, rtol=M.RTOL, atol=M.ATOL)


@pytest.mark.parametrize("name", ["n300_B3", "directed", "no_beta_no_w", "deltaT_half", "single_node"])
def test_marginals_backward_is_the_entry(runs, dev, name):
    """values: the entry's bits; .backward() of the random linear loss: the entry's gradients, grad_w summed over the samples"""
    import torch
    e, out, _, h, n_acc, g, grads, *_ = runs(name)
    tensors = _tensors(CASES[name], dev)
    res = _marginals(e, tensors, deltaT=0.5 if name == "deltaT_half" else 1)
    for c, t in enumerate((res.I, res.S, res.R)):
        assert t.shape == (e.B, e.T, e.n) and t.dtype == torch.float64
        assert torch.equal(t, out[c].view(e.T, e.B, e.n).permute(1, 0, 2))
    gv = [x.view(e.T, e.B, e.n).permute(1, 0, 2) for x in g]
    ((gv[0] * res.I).sum() + (gv[1] * res.S).sum() + (gv[2] * res.R).sum()).backward()
    torch.cuda.synchronize()
    for key, t in zip(("init", "beta", "gamma", "w"), tensors):
        if t is None or t.numel() == 0:
            continue
        want = torch.from_numpy(grads[key]).to(dev)
        if key == "w":
            want = want.sum(0)                                      # the rows' sum, by the same torch op on the same device
        assert t.grad.shape == want.shape and torch.equal(t.grad, want), key


def test_marginals_sum_the_rows_of_shared_rates(runs, dev):
    """[n]-shaped beta and gamma: the values of the expanded rows, and the gradient summed over the samples"""
    import torch
    name = "star260"
    c = dict(CASES[name])
    c["beta"], c["gamma"] = np.repeat(c["beta"][:1], 2, axis=0), np.repeat(c["gamma"][:1], 2, axis=0)
    e = Entry(c, dev)
    out, _, hbuf, n_h, n_acc = e.steps()
    g_host = M.grad_out(c)
    g = torch.from_numpy(np.stack([x.reshape(e.T, e.rows) for x in g_host])).to(dev)
    grads = e.backward(out, hbuf[:n_h].copy(), n_acc, g)
    tensors = _tensors(c, dev, shared_rows=True)
    assert tensors[1].shape == tensors[2].shape == (e.n,)
    res = _marginals(e, tensors)
    assert torch.equal(res.I, out[0].view(e.T, e.B, e.n).permute(1, 0, 2))
    gv = [x.view(e.T, e.B, e.n).permute(1, 0, 2) for x in g]
    ((gv[0] * res.I).sum() + (gv[1] * res.S).sum() + (gv[2] * res.R).sum()).backward()
    for key, t in (("beta", tensors[1]), ("gamma", tensors[2])):
        want = torch.from_numpy(grads[key]).sum(0)                  # torch's sum of the two rows, as autograd's expand does it
        assert t.grad.shape == (e.n,) and torch.equal(t.grad.cpu(), want), key
    assert torch.equal(tensors[3].grad.cpu(), torch.from_numpy(grads["w"]).to(dev).sum(0).cpu())


@pytest.mark.parametrize("form", ["beta_rows", "edge_rates", "beta_and_w"])
def test_marginals_values_are_meanfield_batchs(dev, form):
    import torch
    from gnode.ode_nn import InitialState, edge_rates, meanfield_batch, _meanfield_rates
    c = dict(CASES["directed"])
    e = Entry(c, dev)
    starts = [InitialState(np.ascontiguousarray(c["init"][b])) for b in range(e.B)]
    t = lambda a: torch.from_numpy(np.array(a, np.float64)).to(dev)      # noqa: E731
    kw = dict(deltaT=1, maxTime=e.T, rtol=M.RTOL, atol=M.ATOL)
    from gnode.ode_nn import meanfield_marginals
    if form == "beta_rows":
        want = meanfield_batch(e.g, starts, c["beta"], c["gamma"], **kw)
        got = meanfield_marginals(e.g, t(c["init"]), t(c["beta"]), t(c["gamma"]), None, **kw)
    elif form == "edge_rates":
        want = meanfield_batch(e.g, starts, edge_rates(e.g, c["w"]), c["gamma"], **kw)
        got = meanfield_marginals(e.g, t(c["init"]), None, t(c["gamma"]), t(c["w"]), **kw)
    else:                                                           # both at once: the call behind meanfield_batch
        out, _ = _meanfield_rates(e.g, (c["init"], c["beta"], c["w"], c["gamma"]), e.t_out, M.RTOL, M.ATOL)
        want = [out[k].view(-1, e.B, e.n).permute(1, 0, 2) for k in range(3)]
        got = meanfield_marginals(e.g, t(c["init"]), t(c["beta"]), t(c["gamma"]), t(c["w"]), **kw)
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a, b)


# ------------------------------------------------------------------ refusals: nothing is written
def _refused(e, out, h, n_acc, g, code, text, want=KEYS, short=False, entry=None):
    import torch
    entry = entry or e
    ws = torch.empty(max(e.need(np.max(n_acc, initial=0)), 256), dtype=torch.uint8, device=e.dev)
    grads = entry.grad_buffers(want, fill=7.0)
    rc = entry.call_backward(out, h, n_acc, g, grads, ws, nbytes=(ws.numel() - 1) if short else None)
    torch.cuda.synchronize()
    assert rc == code and text in entry.lib.gnode_last_error().decode(), entry.lib.gnode_last_error().decode()
    for k, v in grads.items():
        assert v is None or bool((v == 7.0).all()), k


def test_refusals_leave_the_gradients_alone(runs, dev):
    e, out, _, h, n_acc, g, *_ = runs("n257")
    _refused(e, out, h, n_acc, g, WORKSPACE, "workspace", short=True)
    _refused(e, out, h, n_acc, g, ARG, "no gradient is asked for", want=())
    x = h.copy()
    x[len(h) // 2] *= 1.5                                           # one h altered: its interval no longer lands on its end
    at = int(np.searchsorted(np.cumsum(n_acc), len(h) // 2, side="right"))
    _refused(e, out, x, n_acc, g, ARG, f"step list, interval {at}: ")
    acc = n_acc.copy()
    acc[-1] -= 1
    _refused(e, out, h, acc, g, ARG, "step list, interval")
    rp, ci = CASES["n257"]["rp"], CASES["n257"]["ci"]               # one directed entry less: the pattern is not symmetric
    k = int(rp[np.argmax(np.diff(rp) >= 3)]) + 1
    rp2 = rp.copy()
    rp2[np.searchsorted(rp, k, side="right"):] -= 1
    c2 = dict(CASES["n257"], w=None)
    lop = Entry(c2, dev, rp=rp2, ci=np.delete(ci, k))
    _refused(e, out, h, n_acc, g, ARG, "not symmetric", entry=lop)
