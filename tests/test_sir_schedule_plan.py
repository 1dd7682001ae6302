"""CPU: the host plan of the scheduled Monte-Carlo call (sir_schedule_layout, sir_stage_schedule of csrc/gnode_sir_plan.cpp),
off the GPU.  Like tests/test_sir_plan.py this module compiles the plan unit with the system g++, here together with
tests/sir_schedule_plan_shim.cpp, loads it with ctypes and checks the layout's offsets, alignment and growth with P, the staged
thresholds per phase, and every refusal with the phase and position in its message."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gn-ode-sir_amd", "csrc")
FIELDS = ["hist", "seeds", "rows", "tail", "thr", "start", "phase", "total", "base_thr", "base_init"]
GRAPHS = [(1, 0, 0), (34, 156, 0), (300, 80, 0), (4096, 16384, 0), (11233, 44932, 0), (76801, 307204, 3), (365825, 1463300, 2)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("sirschedplan")), "libsirschedplan.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(CSRC, "gnode_sir_plan.cpp"), os.path.join(HERE, "sir_schedule_plan_shim.cpp")], check=True)
    L = C.CDLL(so)
    vp, i64 = C.c_void_p, C.c_int64
    L.ssp_layout.restype, L.ssp_layout.argtypes = None, [C.c_int, i64, C.c_int, C.c_int, C.c_int, vp]
    L.ssp_stage.restype, L.ssp_stage.argtypes = C.c_char_p, [C.c_int, i64, C.c_int, C.c_int] + [vp] * 4 + [vp, C.POINTER(i64), vp, C.POINTER(i64)]
    return L


def _layout(lib, n, nnz, nb, T, P):
    o = np.zeros(len(FIELDS), np.int64)
    lib.ssp_layout(n, nnz, nb, T, P, o.ctypes.data)
    return dict(zip(FIELDS, (int(v) for v in o)))


def test_layout_offsets_alignment_and_growth(lib):
    for (n, nnz, nb) in GRAPHS:
        for T in (1, 2, 20):
            prev = None
            for P in (1, 2, 3, 7):
                L = _layout(lib, n, nnz, nb, T, P)
                assert all(L[k] % 256 == 0 for k in FIELDS), (n, nnz, T, P, L)
                # the regions in front of the thresholds are the unscheduled call's
                assert L["thr"] == L["base_thr"] and L["hist"] == 0 and L["hist"] < L["seeds"] < L["rows"] < L["tail"] <= L["thr"]
                assert L["seeds"] - L["hist"] >= 2 * T * n * 4 and L["rows"] - L["seeds"] >= 4096 * 4
                # the P tables, the start thresholds and the phase table follow without overlap
                assert L["start"] - L["thr"] >= P * (nnz + n) * 8
                assert L["phase"] - L["start"] >= 2 * n * 8
                assert L["total"] - L["phase"] >= T * 4
                assert L["start"] - L["thr"] < P * (nnz + n) * 8 + 256 and L["total"] - L["phase"] < max(T, 1) * 4 + 256
                if P == 1:                                          # one phase: the drawn-start form's workspace plus the phase table
                    assert L["phase"] == L["base_init"]
                if prev is not None:
                    assert L["total"] > prev["total"] or (nnz + n) * 8 < 256
                    assert L["total"] - prev["total"] == (L["start"] - L["thr"]) - (prev["start"] - prev["thr"])
                prev = L


def _stage(lib, n, nnz, T, P, phase, W, G, init=None):
    """(error, rates, start)"""
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, t)
    phase, W, G, init = arr(phase, np.int32), arr(W, np.float64), arr(G, np.float64), arr(init, np.float64)
    p = lambda a: None if a is None else a.ctypes.data
    rates, start = np.zeros(max(P, 1) * (nnz + n), np.uint64), np.zeros(2 * n, np.uint64)
    nr, ns = C.c_int64(0), C.c_int64(0)
    err = lib.ssp_stage(n, nnz, T, P, p(phase), p(W), p(G), p(init), rates.ctypes.data, C.byref(nr), start.ctypes.data, C.byref(ns)).decode()
    return err, [int(v) for v in rates[:nr.value]], [int(v) for v in start[:ns.value]]


def coin_threshold(p):
    return int(min(4294967296.0, max(0.0, np.floor(p * 4294967296.0))))


def test_staging_and_refusals(lib):
    thr = lambda a: [coin_threshold(float(x)) for x in np.ravel(a)]
    n, nnz, T, P = 6, 8, 5, 3
    rng = np.random.default_rng(3)
    W, G = rng.uniform(0, 1, (P, nnz)), rng.uniform(0, 1, (P, n))
    W[0, 2], W[1, 3], W[2], G[0, 1], G[2, 4] = 1.0, 0.0, 0.0, 1.0, 0.0
    W[1, 5], G[1, 0] = 2.0 ** -33, 1.0 - 2.0 ** -33
    phase = [7, 0, 2, 1, 2]                                         # entry 0 is never read
    init = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.25, 0.25], [0.2, 0.8, 0.0], [1.0 / 3, 1.0 / 3, 1.0 / 3]])
    # rates = [P][nnz] infection thresholds, then [P][n] recovery thresholds: coin_threshold per phase
    assert _stage(lib, n, nnz, T, P, phase, W, G) == ("", thr(W) + thr(G), [])
    assert _stage(lib, n, nnz, T, P, phase, W, G, init) == ("", thr(W) + thr(G), thr(init[:, 0]) + thr(init[:, 2]))
    assert _stage(lib, n, nnz, T, 1, [0] * T, W[:1], G[:1]) == ("", thr(W[0]) + thr(G[0]), [])
    assert _stage(lib, n, 0, T, 2, [0, 1, 0, 1, 1], np.zeros((2, 0)), G[:2]) == ("", thr(G[:2]), [])          # no entries
    assert _stage(lib, n, nnz, 1, 2, [9], W[:2], G[:2])[0] == ""                                             # T = 1: no step, no phase read
    assert thr([W[1, 5], G[1, 0]]) == [0, 2 ** 32 - 1]

    def refused(*where, **kw):
        a = dict(n=n, nnz=nnz, T=T, P=P, phase=phase, W=W, G=G, init=None)
        a.update(kw)
        err, rates, start = _stage(lib, a["n"], a["nnz"], a["T"], a["P"], a["phase"], a["W"], a["G"], a["init"])
        assert err.startswith("entry: ") and all(w in err for w in where) and (rates, start) == ([], []), (kw, err)

    refused("P = 0", P=0)
    refused("P = -1", P=-1)
    refused("phase[3] = 3", phase=[0, 0, 2, 3, 1])
    refused("phase[1] = -1", phase=[0, -1, 2, 3, 1])
    refused("phase[4] = 1", P=1, phase=[0, 0, 0, 0, 1], W=W[:1], G=G[:1])
    for bad in (float("nan"), -0.1, 1.5):
        x = W.copy(); x[2, 7] = bad; x[2, 6] = 0.5
        refused("phase 2", "position 7", W=x)
        x = W.copy(); x[0, 0] = bad; x[1, 4] = bad
        refused("phase 0", "position 0", W=x)
        x = G.copy(); x[1, 3] = bad; x[2, 0] = bad
        refused("phase 1", "gamma[3]", G=x)
        x = init.copy(); x[3, 1] = bad
        refused("init[3][1]", init=x)
    x = init.copy(); x[4, 1] += 2e-6
    refused("node 4", init=x)
