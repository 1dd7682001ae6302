"""CPU: the Monte-Carlo SIR calls' host plan (csrc/gnode_sir_plan.cpp) is pinned off the GPU.

The plan unit is plain C++; this module compiles it with the system g++ together with tests/sir_plan_shim.cpp, loads the object
with ctypes and checks
  * that every workspace size and offset, the frontier geometry and the path, grid, workgroup size and dynamic LDS of a launch
    are what tests/golden/sir_plan_parent.json recorded from the commit before the plan unit existed (the recipe is in the
    fixture's "recipe" entry), on both sides of every boundary that commit had,
  * coin_threshold, and what the staging function accepts, refuses and says.
`python tests/test_sir_plan.py --cases` prints the case file of the recipe; `python tests/test_sir_plan.py ROWS` turns the
recorder's output into the fixture."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gn-ode-sir_amd", "csrc")
FIXTURE = os.path.join(HERE, "golden", "sir_plan_parent.json")

FIELDS = ["ws_scalar", "ws_nodes", "ws_edges", "ws_init", "ws_traj", "off_seeds", "off_rows", "off_tail", "off_thr", "off_start",
          "lists_in_lds", "frontier_threads", "frontier_per_cu", "frontier_lds", "path", "grid", "threads", "lds"]
FRONTIER_LDS, FRONTIER_MEM, SCAN_LDS, SCAN_MEM = range(4)
COINS = [0.0, 1.0, 2.0 ** -33, 1.0 - 2.0 ** -33, 0.3, 2.0 ** -32, 0.5]
# (n, nnz, n_bigrow): either side of the thread-count switch (4096), the LDS-list bound (11 232 without long rows; long rows
# move it), the 64 KiB of the scan's LDS state (32 768), the scan's LDS-state limit (76 800), the 64 KiB of the frontier's LDS
# (152 832) and the last graph on the frontier path (365 824); a graph of fewer entries than nodes
GRAPHS = [(1, 0, 0), (34, 156, 0), (300, 80, 0), (4095, 16380, 0), (4096, 16384, 0), (11232, 44928, 0), (11233, 44932, 0),
          (11232, 44928, 1), (11228, 44912, 8), (11229, 44916, 8), (32768, 131072, 0), (32769, 131076, 0), (76800, 307200, 0),
          (76801, 307204, 3), (152832, 611328, 0), (152833, 611332, 0), (365824, 1463296, 0), (365825, 1463300, 2),
          (33000, 200000, 0), (153000, 920000, 0)]       # lds64k: the graphs of tests/test_gpu_sir_lds64k.py


def cases():
    """(n, nnz, n_bigrow, T, num_cu, sims, edge_scan)"""
    return [(n, nnz, nb, T, cu, sims, es) for (n, nnz, nb), T, cu, sims, es in
            itertools.product(GRAPHS, (1, 20), (256, 64), (0, 1, 5, 10000), (0, 1))]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("sirplan")), "libsirplan.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(CSRC, "gnode_sir_plan.cpp"), os.path.join(HERE, "sir_plan_shim.cpp")], check=True)
    L = C.CDLL(so)
    vp, i64 = C.c_void_p, C.c_int64
    L.sp_case.restype, L.sp_case.argtypes = None, [C.c_int, i64, C.c_int, C.c_int, C.c_int, i64, C.c_int, vp]
    L.sp_coin.restype, L.sp_coin.argtypes = C.c_uint64, [C.c_double]
    L.sp_stage.restype, L.sp_stage.argtypes = C.c_char_p, [C.c_int, i64, C.c_int, C.c_double, C.c_double] + [vp] * 7 + [C.POINTER(i64), vp, C.POINTER(i64)]
    return L


@pytest.fixture(scope="module")
def parent():
    return json.load(open(FIXTURE))


def _row(lib, case):
    o = np.zeros(len(FIELDS), np.int64)
    lib.sp_case(*case, o.ctypes.data)
    return [int(v) for v in o]


def test_fixture_covers_every_boundary(parent):
    """the recorded rows take the branches the cases were chosen for"""
    assert [tuple(c) for c in parent["cases"]] == cases() and len(parent["rows"]) == len(parent["cases"])
    at = {tuple(c): dict(zip(FIELDS, r)) for c, r in zip(parent["cases"], parent["rows"])}
    row = lambda n, nb=0, T=20, cu=256, sims=10000, es=0: at[next(c for c in at if c[0] == n and c[2:] == (nb, T, cu, sims, es))]
    assert row(4095)["frontier_threads"] == 256 and row(4096)["frontier_threads"] == 512
    assert row(11232)["path"] == FRONTIER_LDS and row(11233)["path"] == FRONTIER_MEM and row(11232, 1)["path"] == FRONTIER_MEM
    assert row(11228, 8)["path"] == FRONTIER_LDS and row(11229, 8)["path"] == FRONTIER_MEM
    assert row(11233)["ws_scalar"] - row(11232)["ws_scalar"] >= 1024 * 3 * 4 * 11233           # the global lists appear
    assert row(32768, es=1)["lds"] == 65536 and row(32769, es=1)["lds"] == 65538 and row(32769, es=1)["path"] == SCAN_LDS
    assert row(76800, es=1)["path"] == SCAN_LDS and row(76801, 3, es=1)["path"] == SCAN_MEM and row(76801, 3, es=1)["lds"] == 0
    assert row(152832)["lds"] <= 65536 < row(152833)["lds"] and row(152833)["path"] == FRONTIER_MEM
    assert row(365824)["path"] == FRONTIER_MEM and row(365825, 2)["path"] == SCAN_MEM
    assert row(300)["ws_nodes"] > row(300)["ws_edges"]                                              # fewer entries than nodes
    assert row(34, cu=64, sims=5)["grid"] == 5 and row(34, sims=0)["grid"] == 0 and row(34, cu=64)["grid"] < row(34)["grid"]
    assert row(365824)["grid"] <= 1024 and row(365825, 2)["grid"] == 2048
    assert row(34, T=1)["off_seeds"] < row(34)["off_seeds"]
    # tests/test_gpu_sir_lds64k.py: each graph takes more than 64 KiB of dynamic LDS on one path and not on the other
    assert (row(33000, es=1)["path"], row(33000, es=1)["lds"], row(33000)["path"], row(33000)["lds"]) == (SCAN_LDS, 66000, FRONTIER_MEM, 20576)
    assert (row(153000)["path"], row(153000)["lds"], row(153000, es=1)["path"], row(153000, es=1)["lds"]) == (FRONTIER_MEM, 65600, SCAN_MEM, 0)


def test_plan_equals_parent(lib, parent):
    for case, want in zip(parent["cases"], parent["rows"]):
        got = _row(lib, case)
        assert got == want, (case, {k: (g, w) for k, g, w in zip(FIELDS, got, want) if g != w})


def test_coin_threshold(lib, parent):
    got = [int(lib.sp_coin(p)) for p in COINS]
    assert got == parent["coins"] == [0, 2 ** 32, 0, 2 ** 32 - 1, int(np.floor(0.3 * 2.0 ** 32)), 1, 2 ** 31]
    assert int(lib.sp_coin(-0.5)) == 0 and int(lib.sp_coin(7.0)) == 2 ** 32                         # clamped, whatever the checks let by


def _stage(lib, n, nnz, form=0, beta=0.3, gamma=0.2, bn=None, gn=None, w=None, col=None, init=None):
    """(error, (tb, tg), rates, start)"""
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, t)
    bn, gn, w, col, init = arr(bn, np.float64), arr(gn, np.float64), arr(w, np.float64), arr(col, np.int32), arr(init, np.float64)
    p = lambda a: None if a is None else a.ctypes.data
    sc, rates, start = np.zeros(2, np.uint64), np.zeros(nnz + n, np.uint64), np.zeros(2 * n, np.uint64)
    nr, ns = C.c_int64(0), C.c_int64(0)
    err = lib.sp_stage(n, nnz, form, beta, gamma, p(bn), p(gn), p(w), p(col), p(init), sc.ctypes.data, rates.ctypes.data, C.byref(nr),
                       start.ctypes.data, C.byref(ns)).decode()
    return err, (int(sc[0]), int(sc[1])), [int(v) for v in rates[:nr.value]], [int(v) for v in start[:ns.value]]


def test_staging(lib):
    thr = lambda a: [int(lib.sp_coin(float(x))) for x in a]
    n, col = 6, [1, 0, 2, 1, 5, 4, 4, 3]
    nnz = len(col)
    rng = np.random.default_rng(3)
    bn, gn, w = rng.uniform(0, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 1, nnz)
    bn[0], gn[1], w[2], w[3] = 0.0, 1.0, 1.0, 0.0
    init = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.25, 0.25], [0.2, 0.8, 0.0], [1.0 / 3, 1.0 / 3, 1.0 / 3]])
    assert _stage(lib, n, nnz) == ("", (thr([0.3])[0], thr([0.2])[0]), [], [])
    assert _stage(lib, n, nnz, 1, bn=bn, gn=gn) == ("", (0, 0), thr(bn) + thr(gn), [])
    assert _stage(lib, n, nnz, 2, w=w, gn=gn) == ("", (0, 0), thr(w) + thr(gn), [])
    assert _stage(lib, n, nnz, 2, w=w, gamma=0.2) == ("", (0, 0), thr(w) + thr([0.2] * n), [])
    assert _stage(lib, n, nnz, 1, bn=bn, gn=gn, col=col, init=init) == ("", (0, 0), thr(bn[col]) + thr(gn), thr(init[:, 0]) + thr(init[:, 2]))
    assert _stage(lib, n, 0, 1, bn=bn, gn=gn, col=np.zeros(1, np.int32)) == ("", (0, 0), thr(gn), [])   # restated with no entries
    assert _stage(lib, n, nnz, init=init)[3] == thr(init[:, 0]) + thr(init[:, 2])
    # refusals name the entry and the first offending index; nothing is staged
    for bad in (float("nan"), -0.1, 1.5):
        def refused(where, **kw):
            err, sc, rates, start = _stage(lib, n, nnz, **kw)
            assert err.startswith("entry: ") and where in err and (rates, start) == ([], []), (bad, kw, err)
        x = bn.copy(); x[4] = bad
        refused("beta[4]", form=1, bn=x, gn=gn)
        refused("beta[4]", form=1, bn=x, gn=gn, col=col)
        x = gn.copy(); x[3] = bad; x[5] = bad
        refused("gamma[3]", form=1, bn=bn, gn=x)
        refused("gamma[3]", form=2, w=w, gn=x)
        x = w.copy(); x[7] = bad
        refused("position 7", form=2, w=x, gn=gn)
        refused("gamma", form=2, w=w, gamma=bad)
        refused("beta", beta=bad)
        refused("gamma", gamma=bad)
        x = init.copy(); x[3, 1] = bad
        refused("init[3][1]", init=x)
    for off, ok in ((2e-6, False), (-2e-6, False), (5e-7, True), (-5e-7, True)):
        x = init.copy(); x[4, 1] += off
        err = _stage(lib, n, nnz, init=x)[0]
        assert (err == "") == ok and (ok or "node 4" in err), (off, err)


RECIPE = ("Recorded from the commit before csrc/gnode_sir_plan.cpp existed, without a GPU: tests/golden/make_sir_plan_parent.cpp "
          "includes that commit's csrc/gnode_sir.hip, stubs gnode_set_error, gn_zero_async, gn_prof_begin, gn_prof_end and "
          "gn_device_setup_once, fills a gnode_graph_s on the stack and calls the exported gnode_sir_*_workspace_bytes functions and the "
          "static planners (frontier_lists_in_lds, frontier_threads, frontier_lds_bytes, coin_threshold); the offsets and the launch "
          "(path, grid, threads, dynamic LDS) are that commit's own expressions from sir_mc_philox_impl, copied next to main.  Built "
          "with `hipcc --offload-arch=gfx950 -O1 -std=c++17 -x hip -Iinclude -Ign-ode-sir_amd/csrc`, run on `python "
          "tests/test_sir_plan.py --cases`, and its output given to `python tests/test_sir_plan.py ROWS`.  rows[i] holds FIELDS of "
          "cases[i] = (n, nnz, n_bigrow, T, num_cu, sims, edge_scan); path 0 / 1 = frontier with lists in LDS / in the workspace, "
          "2 / 3 = scan with state in LDS / in memory; coins = coin_threshold of COINS.")

if __name__ == "__main__":
    if sys.argv[1] == "--cases":
        print("\n".join(" ".join(str(v) for v in c) for c in cases()))
    else:
        lines = open(sys.argv[1]).read().split("\n")
        rows = [[int(v) for v in ln.split()] for ln in lines if ln and not ln.startswith("coin")]
        coins = [int(ln.split()[1]) for ln in lines if ln.startswith("coin")]
        assert len(rows) == len(cases()) and len(coins) == len(COINS)
        with open(FIXTURE, "w") as fh:
            json.dump({"recipe": RECIPE, "fields": FIELDS, "cases": cases(), "coins": coins, "rows": rows}, fh, separators=(",", ":"))
            fh.write("\n")
