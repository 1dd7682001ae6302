#!/usr/bin/env python3
"""RHS value-and-VJP (gnode_rhs_vjp_f32) against the RHS (gnode_rhs_f32) on the same input, and the RK4 adjoint backward
per interval against the Euler backward per interval; device-event timings, one JSON line per case.

Byte model (unique HBM traffic, slabs of rows x H fp32; neighbour rows counted once, as if the gather tables stayed in cache):
  rhs:  MLP reads y_S, y_I, writes Z_S, Z_I (4); gather reads Z_I (table), Z_S, Z_I, beta-gamma, writes dS, dI, dR and the
        zero 4th slab (8)                                                                                    -> 12 slabs
  vjp:  MLP (4); q reads v_S, v_I, Z_S, writes q (4); pass 2 reads the Z_I and q tables, Z_S, Z_I, v_S, v_I, v_R, y_S, y_I,
        beta-gamma (10) and writes f and g_y, 4 slabs each (8)                                               -> 26 slabs
Run on the GPU:  python tools/bench_rhs_vjp.py"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gn-ode-sir_amd"))
import numpy as np, torch
from gnode import _lib, ops, synth
from gnode.graph import DeviceGraph

dev = torch.device("cuda:0")
PEAK = 8.0e12                       # MI355X HBM3E, bytes/s
RHS_SLABS, VJP_SLABS = 12, 26


def ev_ms(fn, reps=20):
    fn(); fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    lib = _lib.load()
    for name, n, m, B, H in (("75k ER x 4", 75000, 300000, 4, 64), ("fb-social size", 1893, 13835, 1, 64)):
        rp, ci = synth.er_csr(n, m, seed=1)
        g = DeviceGraph(rp, ci)
        rows = B * n
        rng = np.random.default_rng(0)
        y = torch.from_numpy(rng.uniform(0, 1.5, size=(4 * rows, H)).astype(np.float32)).to(dev)
        y[3 * rows:, 0], y[3 * rows:, 1] = 0.3, 0.2
        v = torch.randn(4 * rows, H, device=dev)
        P = {k: torch.from_numpy(a).to(dev) for k, a in synth.linear_params(H, seed=2).items()}
        W, b = P["odefunc.linear.weight"], P["odefunc.linear.bias"]
        f, gy = torch.empty_like(y), torch.empty_like(y)
        gW, gb = torch.empty_like(W), torch.empty_like(b)
        wr = torch.empty(lib.gnode_rhs_workspace_bytes(g.handle, rows, H), dtype=torch.uint8, device=dev)
        wv = torch.empty(lib.gnode_rhs_vjp_workspace_bytes(g.handle, rows, H), dtype=torch.uint8, device=dev)
        p = _lib.ptr
        rhs = lambda: _lib.check(lib.gnode_rhs_f32(g.handle, p(y), p(W), p(b), p(f), rows, H, p(wr), wr.numel(), _lib.stream_ptr()))
        vjp = lambda: _lib.check(lib.gnode_rhs_vjp_f32(g.handle, p(y), p(W), p(b), p(v), p(f), p(gy), p(gW), p(gb), rows, H, p(wv),
                                                       wv.numel(), _lib.stream_ptr()))
        t_rhs, t_vjp = ev_ms(rhs), ev_ms(vjp)
        slab = rows * H * 4
        out = {"case": name, "n": n, "B": B, "H": H, "rhs_ms": round(t_rhs, 4), "vjp_ms": round(t_vjp, 4),
               "vjp_over_rhs": round(t_vjp / t_rhs, 2),
               "rhs_TBps": round(RHS_SLABS * slab / (t_rhs * 1e-3) / 1e12, 2), "vjp_TBps": round(VJP_SLABS * slab / (t_vjp * 1e-3) / 1e12, 2),
               "vjp_frac_of_peak": round(VJP_SLABS * slab / (t_vjp * 1e-3) / PEAK, 3)}
        # backward per interval: RK4 vs Euler, 20 grid points (maxTime 10, deltaT 0.5), all outputs
        x = torch.from_numpy(synth.samples(n, B, H, seed=3)).to(dev).reshape(rows, 3 + H)
        dts = ops.step_sizes(ops.time_grid(10, 0.5))
        gs = [torch.randn(len(dts) + 1, rows, device=dev) for _ in range(3)]
        for meth in ("euler", "rk4"):
            sol = ops.forward(g, x, P, dts, meth, None, want_sol=True)[3]
            t = ev_ms(lambda: ops.backward(g, x, P, dts, meth, None, sol, *gs), reps=5)
            out[meth + "_bwd_ms_per_interval"] = round(t / len(dts), 4)
            del sol
        out["rk4_over_euler_bwd"] = round(out["rk4_bwd_ms_per_interval"] / out["euler_bwd_ms_per_interval"], 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
