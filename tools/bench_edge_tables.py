#!/usr/bin/env python3
"""What the entries that read the handle's edge tables (src, rev) cost with one build of libgnode_hip.so, in one process:
tools/bench_dmp_batch.py and tools/bench_dmp_grad.py as they stand (their lines pass through), one gnode_meanfield_rates_f64
call with `w` at er150 size, and gnode_graph_create + gnode_graph_destroy next to one gnode_dmp_batch_f32 call (B = 16, T = 30)
on the same graph at karate size, fb-social size and the size of bench.py's graph.  Medians after a warm-up, wall clock around
a device synchronise.  One JSON line per measurement, tagged "lib": LABEL, appended to --out as well; no threshold.  Two builds
are compared by running this tool on each, alternating (profiles/edge_tables_bench.jsonl: commit 2dc701e as "parent" and the
handle's tables as "here", eight processes each).

    tools/bench_edge_tables.py LIB LABEL [--out FILE]"""
import argparse, contextlib, ctypes as C, io, json, os, runpy, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("gn-ode-sir_amd", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
ap = argparse.ArgumentParser()
ap.add_argument("lib")
ap.add_argument("label")
ap.add_argument("--out", default=None)
opt = ap.parse_args()
LIB, LABEL, OUT = os.path.abspath(opt.lib), opt.label, opt.out
import numpy as np, torch
from gnode import _lib
_lib.LIB_PATH = LIB


def emit(d):
    d = {"lib": LABEL, **d}
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def tool(name):
    buf = io.StringIO()
    sys.argv = [name, "--lib", LIB]
    with contextlib.redirect_stdout(buf):
        runpy.run_path(os.path.join(ROOT, "tools", name), run_name="__main__")
    for ln in buf.getvalue().splitlines():
        if ln.startswith("{"):
            d = json.loads(ln)
            d.pop("lib", None)
            emit({"tool": name, **d})


def med(fn, reps):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


tool("bench_dmp_batch.py")
tool("bench_dmp_grad.py")

import gnode_oracle as O
from gnode import synth
from gnode.graph import DeviceGraph
lib = _lib.load()
dev = torch.device("cuda:0")

# weighted mean-field at er150
rp, ci, _ = O.er_graph(150, 700, seed=1)
n, nnz, B = 150, len(ci), 2
g = DeviceGraph(rp, ci)
rng = np.random.default_rng(3)
init = np.zeros((B, n, 3)); init[:, :, 0] = 1.0; init[:, 5] = (0.0, 1.0, 0.0)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
y0, bet, wd, gam = up(init), up(rng.uniform(0.05, 0.3, (B, n))), up(rng.uniform(0.2, 1.0, nnz)), up(rng.uniform(0.05, 0.4, (B, n)))
t_out = np.arange(8, dtype=np.float64)
out = torch.empty((3, len(t_out), B * n), dtype=torch.float64, device=dev)
ws = torch.empty(lib.gnode_meanfield_rates_workspace_bytes(g.handle, B), dtype=torch.uint8, device=dev)
steps = C.c_int64(-1)


def mf():
    rc = lib.gnode_meanfield_rates_f64(g.handle, B, _lib.ptr(y0), _lib.ptr(bet), _lib.ptr(wd), _lib.ptr(gam), _lib.host_ptr(t_out), len(t_out),
                                       1e-10, 1e-12, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), C.byref(steps), _lib.ptr(ws), ws.numel(),
                                       _lib.stream_ptr())
    assert rc == 0


emit({"tool": "meanfield_rates_w", "case": "er150-size", "n": n, "nnz": nnz, "B": B, "ms": med(mf, 7), "steps": int(steps.value)})

# handle creation, and one gnode_dmp_batch_f32 call (B = 16, T = 30) on the same graph
for name, (rp, ci) in (("karate-size", O.er_graph(34, 78, seed=1)[:2]), ("fb-social-size", O.er_graph(4039, 88234, seed=1)[:2]),
                       ("bench-size", synth.er_csr(75000, 500000, seed=0))):
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
    n, nnz = len(rp) - 1, len(ci)

    def create():
        h = C.c_void_p()
        assert lib.gnode_graph_create(rp.ctypes.data, ci.ctypes.data, n, nnz, C.byref(h)) == 0
        lib.gnode_graph_destroy(h)

    t_create = med(create, 21 if nnz < 200000 else 7)
    g = DeviceGraph(rp, ci)
    Bd, T = 16, 30
    w = torch.full((nnz,), 0.5 / max(1.0, nnz / n), dtype=torch.float32, device=dev)
    gm = torch.full((n,), 0.3, dtype=torch.float32, device=dev)
    st = np.zeros((Bd, n, 3), np.float32); st[:, :, 0] = 1.0; st[:, 3] = (0.0, 1.0, 0.0)
    y = torch.from_numpy(st).to(dev)
    o = torch.empty((Bd, T, n, 3), dtype=torch.float32, device=dev)
    wsd = torch.empty(lib.gnode_dmp_batch_workspace_bytes(g.handle, Bd), dtype=torch.uint8, device=dev)

    def dmp():
        assert lib.gnode_dmp_batch_f32(g.handle, _lib.ptr(w), 0, _lib.ptr(gm), 0, _lib.ptr(y), Bd, T, _lib.ptr(o), _lib.ptr(wsd), wsd.numel(),
                                       _lib.stream_ptr()) == 0

    emit({"tool": "graph_create", "case": name, "n": n, "nnz": nnz, "create_destroy_ms": t_create, "dmp_batch_B16_T30_ms": med(dmp, 5)})
    del g
