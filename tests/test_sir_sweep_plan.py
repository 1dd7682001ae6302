"""CPU: the host plan of the Monte-Carlo candidate sweep (sir_sweep_layout, sir_stage_sweep of csrc/gnode_sir_plan.cpp), off the
GPU.  Like tests/test_sir_schedule_plan.py this module compiles the plan unit with the system g++, here together with
tests/sir_sweep_plan_shim.cpp, loads it with ctypes and checks that the regions are aligned and do not overlap, that the total
is the scheduled call's less the histogram (and the seed list) plus the longer phase row and the two id rows, and every
refusal of the staging with the offending index in its message."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gn-ode-sir_amd", "csrc")
FIELDS = ["rows", "tail", "thr", "start", "phase", "cand", "shifts", "total", "sched_rows", "sched_total", "hist_bytes"]
GRAPHS = [(1, 0, 0), (34, 156, 0), (300, 80, 0), (4096, 16384, 0), (11233, 44932, 0), (76801, 307204, 3), (365825, 1463300, 2)]


def al(x):
    return (x + 255) // 256 * 256


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("sirsweepplan")), "libsirsweepplan.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(CSRC, "gnode_sir_plan.cpp"), os.path.join(HERE, "sir_sweep_plan_shim.cpp")], check=True)
    L = C.CDLL(so)
    vp, i64, i = C.c_void_p, C.c_int64, C.c_int
    L.swp_layout.restype, L.swp_layout.argtypes = None, [i, i64, i, i, i, i, i, vp]
    L.swp_stage.restype, L.swp_stage.argtypes = C.c_char_p, [i, i64, i, i, i, vp, vp, vp, vp, i, vp, C.POINTER(i64), C.POINTER(i64)]
    return L


def _layout(lib, n, nnz, nb, T, P, L, Cn):
    o = np.zeros(len(FIELDS), np.int64)
    lib.swp_layout(n, nnz, nb, T, P, L, Cn, o.ctypes.data)
    return dict(zip(FIELDS, (int(v) for v in o)))


def test_regions_are_aligned_disjoint_and_the_histogram_is_gone(lib):
    for (n, nnz, nb) in GRAPHS:
        for T, L in ((1, 1), (2, 2), (20, 20), (20, 27), (8, 1000)):
            for P in (1, 3):
                for Cn in (1, 5, 64, 1893, 100_000):
                    W = _layout(lib, n, nnz, nb, T, P, L, Cn)
                    assert all(W[k] % 256 == 0 for k in FIELDS), (n, nnz, T, P, L, Cn, W)
                    assert 0 == W["rows"] < W["tail"] <= W["thr"] < W["start"] < W["phase"] < W["cand"] < W["shifts"] < W["total"]
                    # every region holds what lives in it, and ends where the next begins
                    assert W["tail"] - W["rows"] >= max(nnz, 1) * 4
                    assert W["start"] - W["thr"] >= P * (nnz + n) * 8 and W["phase"] - W["start"] >= 2 * n * 8
                    assert W["cand"] - W["phase"] == al(L * 4) and W["shifts"] - W["cand"] == al(Cn * 4) == W["total"] - W["shifts"]
                    # the scheduled call's layout from `rows` on: the histogram and the seed list are gone
                    assert W["hist_bytes"] >= 2 * T * n * 4 and W["sched_rows"] == W["hist_bytes"] + al(4096 * 4)
                    assert W["total"] == W["sched_total"] - W["sched_rows"] - al(T * 4) + al(L * 4) + 2 * al(Cn * 4)
                    if al(L * 4) + 2 * al(Cn * 4) <= al(T * 4) + al(4096 * 4):      # a few candidates: smaller by the histogram at least
                        assert W["total"] <= W["sched_total"] - W["hist_bytes"]


def _stage(lib, n, nnz, T, P, L, phase, W, G, init, Cn, shifts):
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, t)            # noqa: E731
    phase, W, G, init, shifts = arr(phase, np.int32), arr(W, np.float64), arr(G, np.float64), arr(init, np.float64), arr(shifts, np.int32)
    p = lambda a: None if a is None else a.ctypes.data                                # noqa: E731
    nr, ns = C.c_int64(0), C.c_int64(0)
    err = lib.swp_stage(n, nnz, T, P, L, p(phase), p(W), p(G), p(init), Cn, p(shifts), C.byref(nr), C.byref(ns)).decode()
    return err, nr.value, ns.value


def test_staging_and_refusals(lib):
    n, nnz, T, P, L, Cn = 6, 8, 5, 3, 8, 4
    rng = np.random.default_rng(3)
    W, G = rng.uniform(0, 1, (P, nnz)), rng.uniform(0, 1, (P, n))
    phase = [7, 0, 2, 1, 2, 0, 1, 2]                                # entry 0 is never read
    init = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.25, 0.25], [0.2, 0.8, 0.0], [1.0 / 3, 1.0 / 3, 1.0 / 3]])
    good = dict(n=n, nnz=nnz, T=T, P=P, L=L, phase=phase, W=W, G=G, init=init, Cn=Cn, shifts=[0, 3, 1, 3])
    assert _stage(lib, **good) == ("", P * (nnz + n), 2 * n)
    assert _stage(lib, **dict(good, shifts=None)) == ("", P * (nnz + n), 2 * n)    # no shifts: all 0
    assert _stage(lib, **dict(good, L=T, phase=phase[:T], shifts=[0, 0, 0, 0]))[0] == ""
    assert _stage(lib, **dict(good, T=1, L=1, phase=[9], shifts=[0] * 4))[0] == ""  # no step: no phase is read

    def refused(*where, **kw):
        err, nr, ns = _stage(lib, **dict(good, **kw))
        assert err.startswith("entry: ") and all(w in err for w in where) and (nr, ns) == (0, 0), (kw, err)

    refused("shifts[2] = 4", shifts=[0, 3, 4, 9])                   # shift + T > L: the first bad one is named
    refused("shifts[1] = -1", shifts=[0, -1, 0, 0])
    refused("shifts[3] = 1", L=T, phase=phase[:T], shifts=[0, 0, 0, 1])
    refused("L = 4", "T = 5", L=4, phase=phase[:4], shifts=None)
    refused("L = 4", "T = 5", L=4, phase=phase[:4], shifts=[0, 0, 0, 0])
    bad = list(phase); bad[6] = 3                                   # beyond T, inside L: read by a shifted candidate
    refused("phase[6] = 3", phase=bad)
    refused("phase[6] = 3", phase=bad, shifts=None)                 # ... and refused whether or not a shift reaches it
    bad = list(phase); bad[7] = -1
    refused("phase[7] = -1", phase=bad)
    refused("P = 0", P=0)
    x = W.copy(); x[2, 7] = 1.5
    refused("phase 2", "position 7", W=x)
    x = G.copy(); x[1, 3] = float("nan")
    refused("phase 1", "gamma[3]", G=x)
    x = init.copy(); x[3, 1] = -0.1
    refused("init[3][1]", init=x)
