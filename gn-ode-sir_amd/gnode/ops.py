"""Tensor-level entry points over the C ABI (torch is plumbing: memory + streams)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .graph import DeviceGraph

PARAM_KEYS = ("odefunc.linear.weight", "odefunc.linear.bias", "linearS1.weight", "linearS1.bias",
              "linear3.weight", "linear3.bias", "linearS2.weight", "linearS2.bias")

METHODS = {"euler": 0, "rk4": 1}

# Kept activations for the adjoint backward (include/gnode.h: `keep`): on unless GNODE_KEEP=0, read ONCE at import.
# Cost: 3 * (n_steps + 1) * (rows + 1) * 64 floats on top of the trajectory's 4 slabs per grid point (+75 % activation
# memory: 75k nodes x 8 samples x 59 steps = 36.9 GB of trajectory + 27.6 GB kept); when that allocation fails the
# forward falls back to the recomputing backward's layout (no keep buffer) instead of raising.
KEEP_DEFAULT = os.environ.get("GNODE_KEEP", "1") != "0"
# The persistent one-launch integration of mid-size graphs (csrc/gnode_pers64.hip; include/gnode.h: GNODE_FWD_PER_STEP):
# on unless GNODE_PERSIST=0, read once at import.  Same outputs bit for bit either way.
PERSIST_DEFAULT = os.environ.get("GNODE_PERSIST", "1") != "0"
FWD_PER_STEP = 1


def _fwd_flags(persist: bool | None) -> int:
    """The `flags` argument of the forward / backward entries: GNODE_FWD_PER_STEP unless the persistent launch is allowed."""
    return 0 if (PERSIST_DEFAULT if persist is None else persist) else FWD_PER_STEP


def time_grid(maxTime, deltaT) -> np.ndarray:
    """float64 np.arange(0, maxTime, deltaT): reference ode_nn_ngraph_sim.py:110."""
    return np.arange(0, maxTime, deltaT)


def step_sizes(grid: np.ndarray) -> np.ndarray:
    """fp32 dt_k = t[k+1]-t[k] (a 0-dim float64 tensor times an fp32 state stays fp32)."""
    g = np.asarray(grid, dtype=np.float64)
    return np.ascontiguousarray((g[1:] - g[:-1]).astype(np.float32))


def subsample_rows(maxTime, deltaT) -> np.ndarray:
    """Grid rows get_sir_t_nodes_torch keeps: int(i/deltaT), i < maxTime (ode_nn.py:257-259)."""
    return np.asarray([int(i / deltaT) for i in range(int(maxTime))], dtype=np.int32)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise _lib.GnodeError(f"GN-ODE path is fp32 (got {t.dtype})")
    return t if t.is_contiguous() else t.contiguous()


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _check_adjoint(adjoint, method) -> bool:
    """The solver rule, worded here alone: method is euler | rk4, and adjoint=False (the exact gradient of the solve, DESIGN
    section 7.3) exists for Euler.  Returns `adjoint` as a bool."""
    if method not in METHODS:
        raise _lib.GnodeError(f"unknown method {method!r} (euler | rk4)")
    if not adjoint and method != "euler":
        raise _lib.GnodeError(f"adjoint=False is Euler only (method {method!r}): for RK4 the adjoint gradient is within 3.4e-5 of "
                              "the exact one (DESIGN section 7.3), below fp32 noise, so use adjoint=True")
    return bool(adjoint)


def _solve_call(x2d: torch.Tensor, dts, out_rows, upstream=()):
    """What every solve entry is told about its call: (x2d, dts, out_rows) as the contiguous fp32 / fp32 / int32-or-None the C
    ABI reads, and rows, H, n_steps, n_out.  `upstream` (the backwards' gS, gI, gR) must each be [n_out, rows]."""
    x2d = _f32c(x2d)
    rows, H = x2d.shape[0], x2d.shape[1] - 3
    dts = np.ascontiguousarray(dts, dtype=np.float32)
    n_steps = int(dts.shape[0])
    if out_rows is not None:
        out_rows = np.ascontiguousarray(out_rows, dtype=np.int32)
        n_out = int(out_rows.shape[0])
    else:
        n_out = n_steps + 1
    for t in upstream:
        if tuple(t.shape) != (n_out, rows):
            raise _lib.GnodeError(f"upstream gradient shape {tuple(t.shape)} != {(n_out, rows)}")
    return x2d, dts, out_rows, rows, H, n_steps, n_out


def pack_params(tensors: dict) -> _lib.Params:
    p = _lib.Params()
    for k in PARAM_KEYS:
        t = tensors[k]
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise _lib.GnodeError(f"parameter {k} must be a contiguous fp32 GPU tensor")
        setattr(p, k.replace(".", "_"), t.data_ptr())
    return p


def rhs(graph: DeviceGraph, x: torch.Tensor, W: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """ODEfunc.forward on x [4*rows, H] (ode_nn_ngraph_sim.py:58-96)."""
    lib = _lib.load()
    x = _f32c(x)
    graph.check_device(x)
    rows4, H = x.shape
    if rows4 % 4:
        raise _lib.GnodeError("state must have 4 slabs")
    rows = rows4 // 4
    dx = torch.empty_like(x)
    ws = _workspace(lib.gnode_rhs_workspace_bytes(graph.handle, rows, H), x.device)
    _lib.check(lib.gnode_rhs_f32(graph.handle, _lib.ptr(x), _lib.ptr(_f32c(W)), _lib.ptr(_f32c(b)), _lib.ptr(dx), rows, H,
                                 _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    return dx


def rhs_vjp(graph: DeviceGraph, y: torch.Tensor, W: torch.Tensor, b: torch.Tensor, v: torch.Tensor, want_f: bool = False,
            want_y: bool = True, want_W: bool = True, want_b: bool = True):
    """The RHS's vector-Jacobian product at y [4*rows, H] for the cotangent v (same shape): what torch autograd takes through
    ODEfunc.forward (ode_nn_ngraph_sim.py:58-96).  Returns (f or None, dy or None, dW or None, db or None); f (want_f) is
    the RHS itself, bit-identical to `rhs`."""
    lib = _lib.load()
    y, v, W, b = _f32c(y), _f32c(v), _f32c(W), _f32c(b)
    graph.check_device(y)
    if tuple(v.shape) != tuple(y.shape):
        raise _lib.GnodeError(f"cotangent shape {tuple(v.shape)} != state shape {tuple(y.shape)}")
    rows4, H = y.shape
    if rows4 % 4:
        raise _lib.GnodeError("state must have 4 slabs")
    rows = rows4 // 4
    f = torch.empty_like(y) if want_f else None
    dy = torch.empty_like(y) if want_y else None
    dW = torch.empty((H, H), dtype=torch.float32, device=y.device) if want_W else None
    db = torch.empty((H,), dtype=torch.float32, device=y.device) if want_b else None
    ws = _workspace(lib.gnode_rhs_vjp_workspace_bytes(graph.handle, rows, H), y.device)
    _lib.check(lib.gnode_rhs_vjp_f32(graph.handle, _lib.ptr(y), _lib.ptr(W), _lib.ptr(b), _lib.ptr(v), _lib.ptr(f), _lib.ptr(dy),
                                     _lib.ptr(dW), _lib.ptr(db), rows, H, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    return f, dy, dW, db


def forward(graph: DeviceGraph, x2d: torch.Tensor, params: dict, dts: np.ndarray, method: str = "euler",
            out_rows: np.ndarray | None = None, want_sol: bool = False, workspace: torch.Tensor | None = None,
            want_keep: bool | None = None, persist: bool | None = None):
    """ODEBlock.forward on x2d [rows, 3+H]; returns (S, I, R) each [n_out, rows] and sol or None.

    With want_sol (training) and want_keep, the kept activations the adjoint backward reads back (include/gnode.h: `keep`)
    ride along as ``sol.gnode_keep`` (None on paths that keep nothing); `backward` picks them up from there."""
    lib = _lib.load()
    x2d, dts, out_rows, rows, H, n_steps, n_out = _solve_call(x2d, dts, out_rows)
    graph.check_device(x2d)
    m = METHODS[method]
    dev = x2d.device
    out = torch.empty((3, n_out, rows), dtype=torch.float32, device=dev)
    sol = torch.empty((n_steps + 1, 4 * rows, H), dtype=torch.float32, device=dev) if want_sol else None
    need = lib.gnode_forward_workspace_bytes(graph.handle, rows, H, m)
    ws = workspace if (workspace is not None and workspace.numel() >= need) else _workspace(need, dev)
    p = pack_params(params)
    keep = None
    if want_keep is None:
        want_keep = KEEP_DEFAULT
    if sol is not None and want_keep and m == 0:
        kb = lib.gnode_forward_keep_bytes(graph.handle, rows, H, n_steps, n_out)
        if kb:
            try:
                keep = torch.empty(kb // 4, dtype=torch.float32, device=dev)
            except torch.cuda.OutOfMemoryError:
                keep = None                      # the recomputing backward needs only the trajectory
    info = C.c_int32(0)
    _lib.check(lib.gnode_forward_f32(
        graph.handle, _lib.ptr(x2d), C.byref(p), _lib.host_ptr(dts), n_steps, m,
        _lib.host_ptr(out_rows) if out_rows is not None else None, n_out,
        _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.ptr(sol) if sol is not None else None,
        _lib.ptr(keep) if keep is not None else None, keep.numel() * 4 if keep is not None else 0,
        rows, H, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(),
        _fwd_flags(persist), C.byref(info)))
    if sol is not None:
        sol.gnode_keep = keep
        sol.gnode_info = int(info.value)         # what the call left in sol / keep: the backward checks the pairing
    # (no reference to `graph` is kept: a DeviceGraph released while some stream is capturing would hipFree inside the capture)
    forward.last_workspace = (rows, H, m, ws, forward_path(graph, rows, H, n_steps, n_out, sol is not None, method, persist)[0])
    return out[0], out[1], out[2], sol


def forward_path(graph: DeviceGraph, rows: int, H: int, n_steps: int, n_out: int | None = None, want_sol: bool = False,
                 method: str = "euler", persist: bool | None = None):
    """(path, plan): 0 = one launch per Euler step, 1 = one-workgroup launch (tiny graphs), 2 = persistent launch with
    plan = (tiles per workgroup, workgroups per sample, XCDs per sample, samples per XCD, samples alive at once)."""
    plan = (C.c_int32 * 8)()
    path = _lib.load().gnode_forward_path(graph.handle, rows, H, METHODS[method], n_steps, n_steps + 1 if n_out is None else n_out,
                                          int(want_sol), _fwd_flags(persist), plan)
    return int(path), tuple(int(v) for v in plan[:5])


def forward_status() -> int:
    """0, or the give-up code of the persistent launch behind the LAST `forward` call (synchronises the stream)."""
    last = getattr(forward, "last_workspace", None)
    if last is None:
        return 0
    rows, H, m, ws, path = last
    if path not in (2, 3):
        return 0                                 # (the control block is only written by the persistent launch)
    code = C.c_int32(0)
    _lib.check(_lib.load().gnode_forward_status(rows, H, m, _lib.ptr(ws), _lib.stream_ptr(), C.byref(code)))
    return int(code.value)


def _grad_buffers(params: dict, want_params: bool, want_x: bool, x2d: torch.Tensor):
    """(grads dict, packed gradient pointers or None, gx or None): what a backward call writes."""
    grads = {k: torch.empty_like(params[k], memory_format=torch.contiguous_format) for k in PARAM_KEYS} if want_params else {}
    gx = torch.empty_like(x2d) if want_x else None
    if gx is not None:
        grads["x"] = gx
    return grads, (pack_params({k: grads[k] for k in PARAM_KEYS}) if want_params else None), gx


def _run_backward(size_fn: str, entry: str, dx_entry, arrange, graph: DeviceGraph, x2d, params: dict, dts, out_rows, sol,
                  gS, gI, gR, want_x: bool, want_params: bool):
    """One backward call of the library, whichever gradient it is: size_fn sizes its workspace, `entry` is called with
    arrange(head, ups, tail, gx) -- head = (graph, x, params, dts, n_steps, out_rows, n_out, sol), ups = (gS, gI, gR, gradient
    pointers), tail = (rows, H, workspace, its bytes, stream), in the order that entry declares them -- and with want_x
    `dx_entry` is called instead, gx appended (None: `entry` places gx itself).  Returns (grads, (rows, H, workspace))."""
    lib = _lib.load()
    x2d, dts, out_rows, rows, H, n_steps, n_out = _solve_call(x2d, dts, out_rows, (gS, gI, gR))
    grads, gp, gx = _grad_buffers(params, want_params, want_x, x2d)
    ws = _workspace(getattr(lib, size_fn)(graph.handle, rows, H), x2d.device)
    p = pack_params({k: v.detach() for k, v in params.items()})
    args = arrange((graph.handle, _lib.ptr(x2d), C.byref(p), _lib.host_ptr(dts), n_steps,
                    _lib.host_ptr(out_rows) if out_rows is not None else None, n_out, _lib.ptr(_f32c(sol))),
                   (_lib.ptr(_f32c(gS)), _lib.ptr(_f32c(gI)), _lib.ptr(_f32c(gR)), C.byref(gp) if gp is not None else None),
                   (rows, H, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), _lib.ptr(gx))
    if want_x and dx_entry is not None:
        _lib.check(getattr(lib, dx_entry)(*args, _lib.ptr(gx)))
    else:
        _lib.check(getattr(lib, entry)(*args))
    return grads, (rows, H, ws)


def backward(graph: DeviceGraph, x2d: torch.Tensor, params: dict, dts: np.ndarray, method: str, out_rows, sol: torch.Tensor,
             gS: torch.Tensor, gI: torch.Tensor, gR: torch.Tensor, keep="auto", persist: bool | None = None,
             want_x: bool = False, want_params: bool = True, adjoint: bool = True) -> dict:
    """Adjoint parameter gradients (torchdiffeq odeint_adjoint semantics: Euler; rk4)
    given the saved trajectory `sol` and the upstream gradients of S, I, R ([n_out, rows]).
    keep: the forward's kept activations ("auto": ``sol.gnode_keep`` when `forward` attached it; None: recompute; method
    'euler' alone keeps any).
    want_x: also dL/dx2d as key "x" ([rows, 3+H]; include/gnode.h gnode_backward_dx_f32; needs a trajectory produced
    without keep); want_params=False: no parameter gradients (then want_x must be set).
    adjoint=False: the exact gradient of the Euler solve instead (backpropagation through the solver, include/gnode.h
    gnode_backward_discrete_keep_f32).  An EXPLICIT keep=<tensor> (the forward's ``sol.gnode_keep``)
    selects the kept / persistent sweep at H = 64; "auto" and None pass no buffer, so a keep-produced trajectory is refused;
    `persist` is honoured as for the adjoint (H <= 32: the one-launch sweep).  With NEITHER keep nor persist given the call is
    the recomputing one it always was, bit for bit (so its parameter gradients still equal a want_x call's).  `discrete_path`
    says which form runs."""
    if not (want_x or want_params):
        raise _lib.GnodeError("backward: neither parameter nor input gradients requested")
    solve = (graph, x2d, params, dts, out_rows, sol, gS, gI, gR)
    if not _check_adjoint(adjoint, method):
        if isinstance(keep, str):
            # no buffer is picked up from `sol`; with persist left alone too this is the recomputing call of ABI 224, bit for bit
            keep, persist = None, (False if persist is None else persist)
        return _backward_discrete(*solve, want_x=want_x, want_params=want_params, keep=keep, persist=persist)
    if method == "rk4":
        return _backward_rk4(*solve, want_x=want_x, want_params=want_params)
    if isinstance(keep, str):
        keep = getattr(sol, "gnode_keep", None)
    elif keep is None and getattr(sol, "gnode_keep", None) is not None and x2d.shape[1] - 3 == 64:
        # (a trajectory produced WITH kept activations does not carry A Z_I in its 4th slabs: include/gnode.h)
        raise _lib.GnodeError("this trajectory was produced with a keep buffer: pass it (keep='auto'), or run the forward with want_keep=False")
    kept = (_lib.ptr(keep), keep.numel() * 4) if keep is not None else (None, 0)
    last = (_fwd_flags(persist), int(getattr(sol, "gnode_info", -1)))
    grads, backward.last_workspace = _run_backward(
        "gnode_backward_workspace_bytes", "gnode_backward_f32", "gnode_backward_dx_f32",
        lambda head, ups, tail, gx: head + kept + ups + tail + last, *solve, want_x, want_params)
    return grads


def _backward_rk4(graph: DeviceGraph, x2d, params: dict, dts, out_rows, sol, gS, gI, gR, want_x: bool = False,
                  want_params: bool = True) -> dict:
    """The RK4 (3/8 rule) adjoint of a method='rk4' forward: gnode_backward_rk4_f32 (want_x: gnode_backward_rk4_dx_f32)."""
    grads, _ = _run_backward("gnode_backward_rk4_workspace_bytes", "gnode_backward_rk4_f32", "gnode_backward_rk4_dx_f32",
                             lambda head, ups, tail, gx: head + ups + tail,
                             graph, x2d, params, dts, out_rows, sol, gS, gI, gR, want_x, want_params)
    backward.last_workspace = None               # (no persistent sweep on this path: nothing for backward_status to read)
    return grads


def _backward_discrete(graph: DeviceGraph, x2d, params: dict, dts, out_rows, sol, gS, gI, gR, want_x: bool = False,
                       want_params: bool = True, keep=None, persist: bool | None = None) -> dict:
    """The exact gradient of a method='euler' forward: gnode_backward_discrete_keep_f32 (one entry, gx last; the arguments of
    gnode_backward_dx_f32).  keep: the forward's kept activations or None; persist: as `backward`."""
    kept = (_lib.ptr(keep), keep.numel() * 4) if keep is not None else (None, 0)
    last = (_fwd_flags(persist), int(getattr(sol, "gnode_info", -1)))
    # (the call zeroes its control block: backward_status reads 0 unless a persistent sweep gave up)
    grads, backward.last_workspace = _run_backward(
        "gnode_backward_discrete_workspace_bytes", "gnode_backward_discrete_keep_f32", None,
        lambda head, ups, tail, gx: head + kept + ups + tail + last + (gx,),
        graph, x2d, params, dts, out_rows, sol, gS, gI, gR, want_x, want_params)
    return grads


def discrete_path(graph: DeviceGraph, rows: int, H: int, n_steps: int, out_rows=None, sol=None, keep=None,
                  persist: bool | None = None, want_x: bool = False) -> int:
    """The form `backward(adjoint=False, keep=keep, persist=persist, want_x=want_x)` takes on `sol` (include/gnode.h
    gnode_backward_discrete_path): 0 = recomputing, one launch per interval; 1 = kept activations, one launch per interval;
    2 = persistent H = 64 sweep; 3 = persistent H <= 32 sweep."""
    if out_rows is not None:
        out_rows = np.ascontiguousarray(out_rows, dtype=np.int32)
    n_out = int(out_rows.shape[0]) if out_rows is not None else n_steps + 1
    path = _lib.load().gnode_backward_discrete_path(graph.handle, rows, H, n_steps,
                                                    _lib.host_ptr(out_rows) if out_rows is not None else None, n_out,
                                                    int(keep is not None), _fwd_flags(persist),
                                                    int(getattr(sol, "gnode_info", -1)), int(want_x))
    if path < 0:
        raise _lib.GnodeError("discrete_path: bad arguments")
    return int(path)


def backward_status() -> int:
    """0, or the give-up code of the persistent adjoint sweep behind the LAST `backward` call (synchronises the stream)."""
    last = getattr(backward, "last_workspace", None)
    if last is None:
        return 0
    rows, H, ws = last
    code = C.c_int32(0)
    _lib.check(_lib.load().gnode_backward_status(rows, H, _lib.ptr(ws), _lib.stream_ptr(), C.byref(code)))
    return int(code.value)


def l1_loss_sum(S: torch.Tensor, I: torch.Tensor, R: torch.Tensor, y: torch.Tensor, t0: int = 1, want_sign: bool = True, sign_scale: float = 1.0):
    """sum over rows, t >= t0, c of |pred_c[t, row] - y[row, t, c]| as a float64 device scalar, and (want_sign)
    sign(pred - y) * sign_scale as fp32 [3, T, rows] -- the loss of ode_nn_ngraph_sim.py:230-234 and its gradient in one launch
    (sign_scale = 1 / element count gives L1Loss's mean gradient as it stands)."""
    lib = _lib.load()
    S, I, R = (_f32c(t.detach()) for t in (S, I, R))
    T = int(S.shape[0])
    rows = S.numel() // max(T, 1)
    if y.dtype not in (torch.float32, torch.float64):
        y = y.to(torch.float32)
    y = y.detach().contiguous()
    if tuple(y.shape) != (rows, T, 3) or any(t.numel() != T * rows for t in (I, R)):
        raise _lib.GnodeError(f"l1_loss_sum: outputs {tuple(S.shape)} vs labels {tuple(y.shape)}")
    dev = S.device
    total = torch.empty((), dtype=torch.float64, device=dev)
    sgn = torch.empty((3, T, rows), dtype=torch.float32, device=dev) if want_sign else None
    ws = _workspace(lib.gnode_l1_loss_workspace_bytes(), dev)
    _lib.check(lib.gnode_l1_loss_scaled_f32(_lib.ptr(S), _lib.ptr(I), _lib.ptr(R), _lib.ptr(y), int(y.dtype == torch.float64), rows, T,
                                            int(t0), _lib.ptr(total), _lib.ptr(sgn) if sgn is not None else None, float(sign_scale),
                                            _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    return total, sgn
