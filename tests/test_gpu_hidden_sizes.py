"""GPU: the hidden sizes and row counts the rest of the suite does not reach, against float64.

1. H = 68, 100, 124: LPR = gn_lpr(H) = 32 below H = 128, so these run the LPR-32 instances of the generic kernels
   (k_prologue_generic, k_step_generic with and without hub rows, k_mlp_generic, k_bwd_mlp -- above 64 KB of dynamic LDS
   at H = 124 -- and the non-quad k_rhs_vjp), with 15 (H = 68) down to 1 (H = 124) idle lanes per row.
2. Row counts past the point where a capped grid wraps: each workgroup of those launches walks a second row tile and
   carries its partial gradients across it.  The wrap points are derived below from the launchers' formulas; every case
   asserts that its row count is at least twice each one and ragged against both the rows per pass and the wrap point, so
   a later change of grid size fails a guard here instead of silently losing the coverage.

Bars are the suite's: forward 1e-5 against the fp32 C oracle (<= 20 steps) or the numpy oracle (RK4); RHS / VJP 1e-5
(f, dy) and 1e-4 (dW, db) against the float64 restatement; backward 2e-4 per parameter against float64, relative to
the parameter's own largest gradient with the floor at 1e-3 of the overall scale.  Every case also asserts that the
float64 gradients it checks are not degenerate (each parameter's max |grad| above 1e-3 of the overall scale).  No case
needs the fp32 noise-floor rule of test_forward_vs_oracle: at these sizes and horizons (<= 8 steps) a float32 run of the
same oracles sits within 2e-5 of float64, ten times inside the backward bar."""
import numpy as np
import pytest

import fixture_cases as FC
import gnode_restate as RS

pytestmark = pytest.mark.gpu

BWD_NWG = 768            # csrc/gnode_bwd.h: partial-gradient slots, the cap of every lane-group backward grid
GN_HUB_T = 96            # csrc/gnode_common.h: rows longer than this are hub rows
FWD_TOL, VJP_Y_TOL, VJP_W_TOL, BWD_TOL = 1e-5, 1e-5, 1e-4, 2e-4


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30)


def _tp(P, dev):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in P.items()}


def _lpr(H):
    """gn_lpr (csrc/gnode_common.h): lanes per row, H/4 rounded up to a power of two."""
    lpr = 1
    while lpr < H // 4:
        lpr *= 2
    return lpr


# --------------------------------------------------------------------------- wrap points
def _wraps(kernels, H, cu):
    """{kernel: (rows per pass, rows above which its grid wraps)} from the launchers' grid formulas."""
    rpw = 256 // _lpr(H)
    table = {
        # gn_launch_mlp128 (gnode_h128.hip): min(tiles, 2 CU) workgroups over 16-row tiles of the 2*rows S, I rows
        "k_mlp128": (8, 2 * cu * 16 // 2),
        # gn_launch_bwd_mlp128: min(tiles, CU, BWD_NWG) workgroups over 16-row tiles
        "k_bwd_mlp128": (16, min(cu, BWD_NWG) * 16),
        # backward_generic (gnode_bwd.hip): BWD_NWG workgroups of 256 / LPR rows
        "k_bwd_mlp": (rpw, BWD_NWG * rpw),
        # backward_small_h, gn_launch_head_bwd, gn_launch_enc_bwd, vjp_grid (gnode_rhs_vjp.hip): min(BWD_NWG, row groups)
        "k_bwd_fused_generic": (rpw, BWD_NWG * rpw),
        "k_head_bwd": (rpw, BWD_NWG * rpw),
        "k_enc_bwd": (rpw, BWD_NWG * rpw),
        "k_rhs_vjp": (rpw, BWD_NWG * rpw),
    }
    return {k: table[k] for k in kernels}


def _assert_past_wraps(rows, H, kernels):
    import torch
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    for k, (per_pass, wrap) in _wraps(kernels, H, cu).items():
        print(f"[wrap] H={H} {k}: wraps above {wrap} rows, running {rows}")
        assert rows >= 2 * wrap, f"{k}: {rows} rows no longer reach twice the wrap point {wrap} (H={H}, {cu} CUs)"
        assert rows % per_pass and rows % wrap, f"{k}: {rows} rows are not a ragged tail"


# --------------------------------------------------------------------------- inputs and float64 oracles
def _graph(kind, n, m, seed):
    import gnode_oracle as O
    from gnode import synth
    if kind == "er":
        return synth.er_csr(n, m, seed=seed)
    rp, ci, _ = O.chung_lu_graph(n, m, seed=seed)
    assert int(np.diff(rp).max()) > GN_HUB_T                      # hub rows present
    return rp, ci


def _inputs(kind, n, m, B, H, seed, w_scale=1.0, beta_scale=1.0):
    """Graph, parameters and samples.  w_scale shrinks W (dense and hub rows: keeps the sigmoid pre-activations out of
    saturation, where dpre ~ 0 would test nothing); beta_scale slows the hub rows' infection (no stiff Euler steps)."""
    import gnode_oracle as O
    rp, ci = _graph(kind, n, m, seed)
    P = O.init_params(H, seed=seed + 1)
    P["odefunc.linear.weight"] = (P["odefunc.linear.weight"] * w_scale).astype(np.float32)
    x = O.make_samples(n, B, H, seed=seed + 2)
    x[..., 3] *= beta_scale
    return rp, ci, P, x


def _cotangents(n_out, rows, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(n_out, rows)).astype(np.float32) for _ in range(3)]


def euler_oracle(rp, ci, P, x, maxTime, deltaT, gs, out_rows):
    import gnode_oracle as O
    return O.adjoint_grads_torch(x, P, rp, ci, maxTime, deltaT, *gs, out_rows=out_rows, dtype="float64")


def rk4_oracle(rp, ci, P, x, maxTime, deltaT, gs, out_rows):
    import gnode_oracle as O
    grads = RS.adjoint(x.reshape(-1, x.shape[-1]), P, (rp, ci), O.step_sizes(O.time_grid(maxTime, deltaT)),
                       RS.linear_loss(*gs, out_rows), "rk4")
    del grads["x"]
    return grads


def check_grads(got, want, tag):
    """Per parameter: max |got - want| / max(max |want_k|, 1e-3 * scale) <= 2e-4, after the sensitivity guard."""
    scale = max(float(np.abs(w).max()) for w in want.values())
    for k, w in want.items():
        g = got[k].cpu().numpy().astype(np.float64)
        if k == "linearS2.bias":                                   # exact gradient 0 (softmax shift invariance)
            assert abs(float(g[0])) <= 1e-4 * max(1.0, float(np.abs(want["linearS2.weight"]).max())), f"{tag}: {k}"
            continue
        peak = float(np.abs(w).max())
        assert peak > 1e-3 * scale, f"{tag}: {k} is degenerate in this case ({peak:.2e} vs scale {scale:.2e})"
        err = float(np.max(np.abs(g - w))) / (max(peak, 1e-3 * scale) + 1e-30)
        print(f"[grad] {tag}: {k} rel err {err:.2e}")
        assert err <= BWD_TOL, f"{tag}: {k} rel err {err:.2e}"


def _forward(dev, rp, ci, P, x, grid, method, out_rows=None, want_sol=False, want_keep=None):
    import torch
    from gnode import ops
    from gnode.graph import DeviceGraph
    B, n, H = x.shape[0], x.shape[1], x.shape[2] - 3
    g = DeviceGraph(rp, ci)
    params = _tp(P, dev)
    x2d = torch.from_numpy(x).to(dev).reshape(B * n, 3 + H)
    dts = ops.step_sizes(grid)
    S, I, R, sol = ops.forward(g, x2d, params, dts, method, out_rows, want_sol=want_sol, want_keep=want_keep)
    return g, params, x2d, dts, (S, I, R), sol


def _check_forward(dev, rp, ci, P, x, maxTime, deltaT, method, tag):
    import gnode_oracle as O
    import oracle_c as OC
    from gnode import ops
    grid = O.time_grid(maxTime, deltaT)
    assert len(grid) - 1 <= 20                                      # fp32 reproducible to 1e-5 on this horizon
    B, n, H = x.shape[0], x.shape[1], x.shape[2] - 3
    g, _, _, _, got, _ = _forward(dev, rp, ci, P, x, grid, method)
    assert ops.forward_path(g, B * n, H, len(grid) - 1, method=method)[0] == 0      # one launch per step
    if method == "euler":
        want = OC.forward_euler(rp, ci, n, x, P, O.step_sizes(grid))
    else:
        want = O.odeblock_forward_single(x, P, rp, ci, maxTime, deltaT, method="rk4")
    for c, a, w in zip("SIR", got, want):
        err = _rel(a.cpu().numpy(), w[..., 0])
        print(f"[fwd] {tag} {c}: rel err {err:.2e}")
        assert err <= FWD_TOL, f"{tag} {c}: rel err {err:.2e}"


def _check_backward(dev, rp, ci, P, x, maxTime, deltaT, method, out_rows, tag):
    """GPU backward against the float64 oracle: over the kept activations where the forward keeps any, and recomputing."""
    import gnode_oracle as O
    from gnode import ops
    import torch
    grid = O.time_grid(maxTime, deltaT)
    B, n = x.shape[0], x.shape[1]
    rows = B * n
    n_out = len(grid) if out_rows is None else len(out_rows)
    gs = _cotangents(n_out, rows)
    want = (euler_oracle if method == "euler" else rk4_oracle)(rp, ci, P, x, maxTime, deltaT, gs, out_rows)
    g, params, x2d, dts, _, sol = _forward(dev, rp, ci, P, x, grid, method, out_rows, want_sol=True)
    gst = [torch.from_numpy(a).to(dev) for a in gs]
    kept = getattr(sol, "gnode_keep", None) is not None
    variants = {"kept" if kept else "recomputed": ops.backward(g, x2d, params, dts, method, out_rows, sol, *gst)}
    if kept:
        _, _, _, _, _, sol_nk = _forward(dev, rp, ci, P, x, grid, method, out_rows, want_sol=True, want_keep=False)
        variants["recomputed"] = ops.backward(g, x2d, params, dts, method, out_rows, sol_nk, *gst)
    for name, got in variants.items():
        check_grads(got, want, f"{tag} {name}")


# --------------------------------------------------------------------------- 1. H = 68, 100, 124 (LPR = 32 below H = 128)
MID = {
    68: ("er", 500, 3000, 2, 1.0, 1.0),
    100: ("er", 500, 3000, 2, 1.0, 1.0),
    124: ("cl", 2000, 20000, 2, 0.2, 0.05),          # hub rows: W and beta scaled down (saturation, stiffness)
}


@pytest.mark.parametrize("H", [68, 100, 124])
def test_euler_forward_mid_h(H, dev):
    """k_prologue_generic<32> and k_step_generic<32, false> (ER), <32, true> and the hub segments (Chung-Lu, H = 124)."""
    kind, n, m, B, ws, bs = MID[H]
    rp, ci, P, x = _inputs(kind, n, m, B, H, seed=H, w_scale=ws, beta_scale=bs)
    _check_forward(dev, rp, ci, P, x, 4, 0.5, "euler", f"H={H} {kind}")


def test_rk4_forward_h100(dev):
    """k_mlp_generic<32> in every RK4 stage."""
    rp, ci, P, x = _inputs("er", 500, 3000, 2, 100, seed=7)
    _check_forward(dev, rp, ci, P, x, 3, 0.5, "rk4", "rk4 H=100")


@pytest.mark.parametrize("kind,H", [("er", 68), ("cl", 124)])
def test_rhs_and_vjp_mid_h(kind, H, dev):
    """gnode_rhs_f32 (k_mlp_generic<32>) and gnode_rhs_vjp_f32 (k_rhs_vjp<32, false>: 256 % H != 0)."""
    n, m, B = (400, 2000, 3) if kind == "er" else (2000, 20000, 2)
    rp, ci = _graph(kind, n, m, seed=H)
    _rhs_vjp_case(dev, rp, ci, n, B, H, f"{kind} H={H}", w_scale=1.0 if kind == "er" else 0.2)


def _rhs_vjp_case(dev, rp, ci, n, B, H, tag, w_scale=1.0):
    import torch
    from gnode import ops, synth
    from gnode.graph import DeviceGraph
    y, v = FC.vjp_inputs(B * n, H, seed=H, sample_rows=n)
    P = synth.linear_params(H, seed=H + 7)
    W = (P["odefunc.linear.weight"] * w_scale).astype(np.float32)
    b = P["odefunc.linear.bias"]
    wf, wy, wW, wb = RS.rhs_vjp_np(y, W, b, v, rp, ci)
    for name, w in (("dW", wW), ("db", wb)):                    # sensitivity: dpre is not ~0 everywhere
        assert float(np.abs(w).max()) > 1e-3 * float(np.abs(wy).max()), f"{tag}: {name} degenerate"
    g = DeviceGraph(rp, ci)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    yt, vt, Wt, bt = t(y), t(v), t(W), t(b)
    f, gy, gW, gb = ops.rhs_vjp(g, yt, Wt, bt, vt, want_f=True)
    fr = ops.rhs(g, yt, Wt, bt)
    errs = {"rhs": _rel(fr.cpu().numpy(), wf), "f": _rel(f.cpu().numpy(), wf), "dy": _rel(gy.cpu().numpy(), wy),
            "dW": _rel(gW.cpu().numpy(), wW), "db": _rel(gb.cpu().numpy(), wb)}
    print(f"[vjp] {tag}: " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert errs["rhs"] <= VJP_Y_TOL and errs["f"] <= VJP_Y_TOL and errs["dy"] <= VJP_Y_TOL, (tag, errs)
    assert errs["dW"] <= VJP_W_TOL and errs["db"] <= VJP_W_TOL, (tag, errs)
    assert torch.equal(f, fr)


@pytest.mark.parametrize("sub", [False, True], ids=["full", "subsampled"])
@pytest.mark.parametrize("H", [68, 100, 124])
def test_euler_backward_mid_h(H, sub, dev):
    """The five-launch generic backward at LPR = 32: k_bwd_gather<32>, k_bwd_mlp<32> (> 64 KB of LDS at H = 124),
    k_head_bwd<32>, k_enc_bwd<32>; with and without the fused out_rows subsample."""
    from gnode import ops
    kind, n, m, B, ws, bs = MID[H]
    if kind == "cl":
        n, m = 600, 6000
    rp, ci, P, x = _inputs(kind, n, m, B, H, seed=H, w_scale=ws, beta_scale=bs)
    out_rows = ops.subsample_rows(3, 0.5) if sub else None
    _check_backward(dev, rp, ci, P, x, 3, 0.5, "euler", out_rows, f"euler H={H} {kind} sub={sub}")


def test_rk4_backward_h100(dev):
    """The RK4 adjoint at LPR = 32: k_rhs_vjp<32, false> in every stage, k_mlp_generic<32>."""
    from gnode import ops
    rp, ci, P, x = _inputs("er", 400, 2000, 2, 100, seed=11)
    _check_backward(dev, rp, ci, P, x, 2, 0.5, "rk4", ops.subsample_rows(2, 0.5), "rk4 H=100")


# --------------------------------------------------------------------------- 2. past every wrap point, ragged tails
H128 = ("er", 4999, 25000, 3)                          # 14 997 rows


@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_h128_forward_past_wrap(method, dev):
    kind, n, m, B = H128
    _assert_past_wraps(B * n, 128, ["k_mlp128"])
    rp, ci, P, x = _inputs(kind, n, m, B, 128, seed=128)
    _check_forward(dev, rp, ci, P, x, 2, 0.5, method, f"{method} H=128 rows={B * n}")


@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_h128_backward_past_wrap(method, dev):
    """k_bwd_mlp128 (Euler) and k_rhs_vjp<32, true> (RK4), k_head_bwd<32> and k_enc_bwd<32>, all wrapping."""
    kind, n, m, B = H128
    kernels = ["k_mlp128", "k_head_bwd", "k_enc_bwd"] + (["k_bwd_mlp128"] if method == "euler" else ["k_rhs_vjp"])
    _assert_past_wraps(B * n, 128, kernels)
    rp, ci, P, x = _inputs(kind, n, m, B, 128, seed=128)
    _check_backward(dev, rp, ci, P, x, 2.5, 0.5, method, None, f"{method} H=128 rows={B * n}")


@pytest.mark.parametrize("H,n", [(128, 4999), (124, 6001)])
def test_rhs_vjp_past_wrap(H, n, dev):
    B = 3
    _assert_past_wraps(B * n, H, ["k_rhs_vjp"])
    rp, ci = _graph("er", n, 6 * n, seed=H)
    _rhs_vjp_case(dev, rp, ci, n, B, H, f"H={H} rows={B * n}")


@pytest.mark.parametrize("H,n,B", [(100, 6001, 3), (124, 6001, 3), (48, 8677, 3), (24, 20011, 3), (16, 33343, 3)])
def test_euler_backward_past_wrap(H, n, B, dev):
    """k_bwd_mlp<LPR> (32 < H != 64) or the per-interval k_bwd_fused_generic<LPR> (H <= 32), with k_head_bwd and
    k_enc_bwd, each past its wrap point; out_rows subsampled so that the last interval emits nothing."""
    from gnode import ops
    from gnode.graph import DeviceGraph
    rows = B * n
    kernels = ["k_head_bwd", "k_enc_bwd"] + (["k_bwd_fused_generic"] if H <= 32 else ["k_bwd_mlp"])
    _assert_past_wraps(rows, H, kernels)
    maxTime, deltaT = 2, 0.5
    rp, ci, P, x = _inputs("er", n, 4 * n, B, H, seed=H)
    out_rows = ops.subsample_rows(maxTime, deltaT)
    if H <= 32:          # beyond the persistent small-H sweep's resident grid: the per-interval kernel runs
        n_steps = len(ops.time_grid(maxTime, deltaT)) - 1
        assert ops.forward_path(DeviceGraph(rp, ci), rows, H, n_steps, len(out_rows), want_sol=True)[0] == 0
    _check_backward(dev, rp, ci, P, x, maxTime, deltaT, "euler", out_rows, f"euler H={H} rows={rows}")


# --------------------------------------------------------------------------- 5. the H contract
def test_forward_and_rhs_refuse_h_above_128(dev):
    """4 <= H <= 128 for every GN-ODE entry: the forward (even without steps) and the RHS refuse H = 132."""
    import torch
    from gnode import _lib, ops, synth
    from gnode.graph import DeviceGraph
    import gnode_oracle as O
    n, H = 50, 132
    rp, ci = synth.er_csr(n, 150, seed=1)
    g = DeviceGraph(rp, ci)
    P = _tp(O.init_params(H, seed=0), dev)
    x = torch.from_numpy(O.make_samples(n, 1, H, seed=1)).to(dev).reshape(n, 3 + H)
    with pytest.raises(_lib.GnodeError):
        ops.forward(g, x, P, ops.step_sizes(ops.time_grid(0.5, 0.5)))
    with pytest.raises(_lib.GnodeError):
        ops.forward(g, x, P, ops.step_sizes(ops.time_grid(2, 0.5)))
    with pytest.raises(_lib.GnodeError):
        ops.rhs(g, torch.zeros((4 * n, H), device=dev), P["odefunc.linear.weight"], P["odefunc.linear.bias"])
    assert "128" in _lib.load().gnode_last_error().decode()
