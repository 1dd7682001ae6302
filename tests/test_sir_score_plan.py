"""CPU: the host plan of the Monte-Carlo source scores (sir_score_layout, sir_stage_score and the static-LDS argument of
sir_launch_plan in csrc/gnode_sir_plan.cpp), off the GPU.  Like tests/test_sir_sweep_plan.py this module compiles the plan unit
with the system g++, here together with tests/sir_score_plan_shim.cpp, loads it with ctypes and checks that the regions are
aligned and do not overlap, that the layout is the sweep's with the snapshots and two tables behind it -- the sweep's own
layout unchanged -- that the tallies' static LDS moves the two LDS boundaries and only them, and every refusal of the staging
with the offending index in its message."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gn-ode-sir_amd", "csrc")
FIELDS = ["rows", "tail", "thr", "start", "phase", "cand", "shifts", "obs", "marked", "seen", "total", "sweep_tail", "sweep_thr", "sweep_total"]
PLAN = ["path", "threads", "grid", "lds", "lists_in_lds"]
FRONTIER_LDS, FRONTIER_MEM, SCAN_LDS, SCAN_MEM = range(4)
GRAPHS = [(1, 0, 0), (34, 156, 0), (300, 80, 0), (4096, 16384, 0), (11200, 44800, 0), (11201, 44804, 0), (11232, 44928, 0), (11233, 44932, 0),
          (76736, 307204, 3), (76737, 307204, 3), (76800, 307204, 3), (76801, 307204, 3), (365825, 1463300, 2)]


def al(x):
    return (x + 255) // 256 * 256


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("sirscoreplan")), "libsirscoreplan.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(CSRC, "gnode_sir_plan.cpp"), os.path.join(HERE, "sir_score_plan_shim.cpp")], check=True)
    L = C.CDLL(so)
    vp, i64, i = C.c_void_p, C.c_int64, C.c_int
    L.sco_static_lds.restype = i64
    L.sco_layout.restype, L.sco_layout.argtypes = None, [i, i64, i, i, i, i, i, i, vp]
    L.sco_plan.restype, L.sco_plan.argtypes = None, [i, i, i, i64, i, i64, vp]
    L.sco_stage.restype = C.c_char_p
    L.sco_stage.argtypes = [i, i64, i, i, i, vp, vp, vp, vp, i, vp, vp, i, i, i, vp, vp, vp, C.POINTER(i64), C.POINTER(i64)]
    return L


def _layout(lib, n, nnz, nb, T, P, L, Cn, O):
    o = np.zeros(len(FIELDS), np.int64)
    lib.sco_layout(n, nnz, nb, T, P, L, Cn, O, o.ctypes.data)
    return dict(zip(FIELDS, (int(v) for v in o)))


def _plan(lib, n, nb, jobs, edge_scan, static_lds, cu=256):
    o = np.zeros(len(PLAN), np.int64)
    lib.sco_plan(n, nb, cu, jobs, int(edge_scan), static_lds, o.ctypes.data)
    return dict(zip(PLAN, (int(v) for v in o)))


def test_the_tallies_are_two_int32_per_snapshot(lib):
    assert lib.sco_maxo() == 16 and lib.sco_static_lds() == 2 * 16 * 4


def test_regions_are_aligned_disjoint_and_the_sweeps_with_the_snapshots_behind(lib):
    S = lib.sco_static_lds()
    for (n, nnz, nb) in GRAPHS:
        for T, L in ((1, 1), (20, 27), (8, 1000)):
            for P, Cn in ((1, 1), (3, 1893)):
                for O in (1, 7, 16):
                    W = _layout(lib, n, nnz, nb, T, P, L, Cn, O)
                    assert all(W[k] % 256 == 0 for k in FIELDS), (n, nnz, T, P, L, Cn, O, W)
                    assert 0 == W["rows"] < W["tail"] <= W["thr"] < W["start"] < W["phase"] < W["cand"] < W["shifts"] < W["obs"] < W["marked"] < W["seen"] < W["total"]
                    assert W["obs"] - W["shifts"] == al(Cn * 4)                   # the sweep's regions end where the snapshots begin
                    assert W["marked"] - W["obs"] == al(O * n) and W["seen"] - W["marked"] == al(O * 4) == W["total"] - W["seen"]
                    assert W["tail"] == W["sweep_tail"]
                    # the sweep's own tail, unless the tallies push the lists or the scan's state out of LDS: then it holds them
                    grown = W["thr"] - W["sweep_thr"]
                    lists_moved = _plan(lib, n, nb, 1000, False, 0)["lists_in_lds"] and not _plan(lib, n, nb, 1000, False, S)["lists_in_lds"]
                    state_moved = 2 * n <= 150 * 1024 < 2 * n + S
                    assert (grown > 0) == lists_moved, (n, grown)                  # (the lists' region already holds the scan's state)
                    assert W["obs"] == W["sweep_total"] + grown
                    if lists_moved:
                        assert W["thr"] - W["tail"] >= 1024 * 3 * n * 4
                    if state_moved:
                        assert W["thr"] - W["tail"] >= 2048 * 2 * n


def test_the_static_lds_moves_the_two_boundaries_and_nothing_else(lib):
    S = lib.sco_static_lds()
    # lists in LDS: bitmaps + lists + tallies within 48 KiB -- n = 11 232 without the tallies, 11 200 with them
    assert _plan(lib, 11232, 0, 1000, False, 0)["path"] == FRONTIER_LDS and _plan(lib, 11233, 0, 1000, False, 0)["path"] == FRONTIER_MEM
    assert _plan(lib, 11200, 0, 1000, False, S)["path"] == FRONTIER_LDS and _plan(lib, 11201, 0, 1000, False, S)["path"] == FRONTIER_MEM
    p = _plan(lib, 11200, 0, 1000, False, S)
    assert p["lds"] + S <= 160 * 1024 and p["lds"] >= 3 * 352 * 4 + 2 * 2 * 11200
    assert _plan(lib, 11201, 0, 1000, False, S)["grid"] <= 1024       # a workgroup per set of lists in the workspace
    # the scan's state in LDS: 2 n + tallies within 150 KiB
    assert _plan(lib, 76800, 0, 1000, True, 0)["path"] == SCAN_LDS and _plan(lib, 76801, 0, 1000, True, 0)["path"] == SCAN_MEM
    assert _plan(lib, 76736, 0, 1000, True, S)["path"] == SCAN_LDS and _plan(lib, 76737, 0, 1000, True, S)["path"] == SCAN_MEM
    for n in (1, 34, 300, 4095, 4096, 11000, 20000, 70000, 200000):       # away from the boundaries: the plan it was
        for scan in (False, True):
            a, b = _plan(lib, n, 0, 10**6, scan, 0), _plan(lib, n, 0, 10**6, scan, S)
            assert (a["path"], a["threads"], a["lds"]) == (b["path"], b["threads"], b["lds"]) and b["grid"] <= a["grid"], (n, scan, a, b)
            # the workgroups of a CU and their tallies fit its LDS
            if b["path"] != SCAN_MEM:
                assert -(-b["grid"] // 256) * (b["lds"] + S) <= 160 * 1024


def _stage(lib, n, nnz, T, P, L, phase, W, G, init, Cn, shifts, obs, measure, bins, O=None):
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, t)            # noqa: E731
    phase, W, G, init, shifts = arr(phase, np.int32), arr(W, np.float64), arr(G, np.float64), arr(init, np.float64), arr(shifts, np.int32)
    obs = arr(obs, np.int8)
    O = obs.shape[0] if O is None else O
    p = lambda a: None if a is None else a.ctypes.data                                # noqa: E731
    out, marked, seen = np.full((n, max(O, 1)), 99, np.int8), np.zeros(max(O, 1), np.int32), np.zeros(max(O, 1), np.int32)
    nr, no = C.c_int64(0), C.c_int64(0)
    err = lib.sco_stage(n, nnz, T, P, L, p(phase), p(W), p(G), p(init), Cn, p(shifts), p(obs), O, measure, bins, p(out), p(marked), p(seen),
                        C.byref(nr), C.byref(no)).decode()
    return err, nr.value, no.value, out, marked, seen


def test_staging_and_refusals(lib):
    n, nnz, T, P, L, Cn = 6, 8, 5, 3, 8, 4
    rng = np.random.default_rng(3)
    W, G = rng.uniform(0, 1, (P, nnz)), rng.uniform(0, 1, (P, n))
    phase = [7, 0, 2, 1, 2, 0, 1, 2]
    init = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.25, 0.25], [0.2, 0.8, 0.0], [1.0 / 3, 1.0 / 3, 1.0 / 3]])
    obs = np.asarray([[0, 1, 2, -1, 1, 0], [-1, -1, -1, -1, -1, 0], [2, 2, 2, 2, 2, 2]], np.int8)
    good = dict(n=n, nnz=nnz, T=T, P=P, L=L, phase=phase, W=W, G=G, init=init, Cn=Cn, shifts=[0, 3, 1, 3], obs=obs, measure=0, bins=64)
    err, nr, no, out, marked, seen = _stage(lib, **good)
    assert (err, nr, no) == ("", P * (nnz + n), 3 * n)
    assert np.array_equal(out, obs.T) and marked.tolist() == [3, 0, 6] and seen.tolist() == [5, 1, 6]     # node-major; |A_o|; observed
    assert _stage(lib, **dict(good, measure=1, bins=1, shifts=None))[0] == "" and _stage(lib, **dict(good, bins=4096))[0] == ""
    assert _stage(lib, **dict(good, obs=np.tile(obs[0], (16, 1))))[0] == ""

    def refused(*where, **kw):
        err, nr, no = _stage(lib, **dict(good, **kw))[:3]
        assert err.startswith("entry: ") and all(w in err for w in where) and (nr, no) == (0, 0), (kw, err)

    refused("O = 0", O=0)
    refused("O = 17", obs=np.tile(obs[0], (17, 1)))
    refused("O = -1", O=-1)
    refused("bins = 0", bins=0)
    refused("bins = 4097", bins=4097)
    refused("measure 2", measure=2)
    refused("measure -1", measure=-1)
    x = obs.copy(); x[1, 4] = 3
    refused("obs[1][4] = 3", obs=x)
    x = obs.copy(); x[2, 0] = -2
    refused("obs[2][0] = -2", obs=x)
    x = obs.copy(); x[1, 5] = -1
    refused("snapshot 1 observes no node", obs=x)
    refused("2^31", Cn=200_000, shifts=None, bins=4096, T=2, L=8)                 # 3 x 200 000 x 2 x 4097 cells
    assert _stage(lib, **dict(good, Cn=80_000, shifts=None, bins=4096, T=2, L=8))[0] == ""       # 1.97e9 < 2^31
    # the sweep's refusals, through the same function
    refused("shifts[2] = 4", shifts=[0, 3, 4, 9])
    refused("L = 4", "T = 5", L=4, phase=phase[:4], shifts=None)
    bad = list(phase); bad[6] = 3
    refused("phase[6] = 3", phase=bad)
    x = W.copy(); x[2, 7] = 1.5
    refused("phase 2", "position 7", W=x)
    x = init.copy(); x[3, 1] = -0.1
    refused("init[3][1]", init=x)
