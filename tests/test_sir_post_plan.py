"""CPU: the host plan of the Monte-Carlo nowcast and forecast from timed evidence (sir_post_layout, sir_stage_post and the
static-LDS argument of sir_launch_plan in csrc/gnode_sir_plan.cpp), off the GPU.  Like tests/test_sir_timed_plan.py this module
compiles the plan unit with the system g++, here together with tests/sir_post_plan_shim.cpp, loads it with ctypes and checks
that the regions are aligned and do not overlap, that the layout is the sweep's with the record tables and the horizons behind
it, that the 64 bytes of counters are counted in the launch plan, that the records are staged exactly as sir_stage_timed stages
them, that 16 sets are accepted at T = 2048, and every refusal of the staging with the offending index in its message."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gn-ode-sir_amd", "csrc")
FIELDS = ["rows", "tail", "thr", "start", "phase", "cand", "shifts", "rec_ptr", "rec", "zeros", "records", "horizons", "total", "sweep_tail",
          "sweep_thr", "sweep_total"]
PLAN = ["path", "threads", "grid", "lds", "lists_in_lds"]
FRONTIER_LDS, FRONTIER_MEM, SCAN_LDS, SCAN_MEM = range(4)
GRAPHS = [(1, 0, 0), (34, 156, 0), (300, 80, 0), (4096, 16384, 0), (11216, 44864, 0), (11217, 44868, 0), (11232, 44928, 0), (11233, 44932, 0),
          (76768, 307072, 3), (76769, 307076, 3), (76800, 307204, 3), (76801, 307204, 3), (365825, 1463300, 2)]


def al(x):
    return (x + 255) // 256 * 256


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("sirpostplan")), "libsirpostplan.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(CSRC, "gnode_sir_plan.cpp"), os.path.join(HERE, "sir_post_plan_shim.cpp")], check=True)
    L = C.CDLL(so)
    vp, i64, i = C.c_void_p, C.c_int64, C.c_int
    p64 = C.POINTER(i64)
    L.pst_static_lds.restype = i64
    L.pst_layout.restype, L.pst_layout.argtypes = None, [i, i64, i, i, i, i, i, i, i, i, vp]
    L.pst_plan.restype, L.pst_plan.argtypes = None, [i, i, i, i64, i, i64, vp]
    L.pst_stage.restype, L.pst_stage_timed.restype = C.c_char_p, C.c_char_p
    L.pst_stage.argtypes = [i, i64, i, i, i, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, vp, i, vp, vp, vp, vp, vp, p64, p64, p64]
    L.pst_stage_timed.argtypes = [i, i64, i, i, i, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, p64, p64]
    return L


def _layout(lib, n, nnz, nb, T, P, L, Cn, O, R, H):
    o = np.zeros(len(FIELDS), np.int64)
    lib.pst_layout(n, nnz, nb, T, P, L, Cn, O, R, H, o.ctypes.data)
    return dict(zip(FIELDS, (int(v) for v in o)))


def _plan(lib, n, nb, jobs, edge_scan, static_lds, cu=256):
    o = np.zeros(len(PLAN), np.int64)
    lib.pst_plan(n, nb, cu, jobs, int(edge_scan), static_lds, o.ctypes.data)
    return dict(zip(PLAN, (int(v) for v in o)))


def test_the_counters_are_16_int32_of_static_lds(lib):
    assert lib.pst_maxo() == 16 and lib.pst_maxh() == 32 and lib.pst_static_lds() == 16 * 4


def test_regions_are_aligned_disjoint_and_the_sweeps_with_the_records_and_horizons_behind(lib):
    S = lib.pst_static_lds()
    for (n, nnz, nb) in GRAPHS:
        for T, L in ((1, 1), (20, 27), (2048, 2100)):
            for P, Cn in ((1, 1), (3, 1893)):
                for O, R, H in ((1, 1, 1), (7, 40, 3), (16, 5000, 32)):
                    W = _layout(lib, n, nnz, nb, T, P, L, Cn, O, R, H)
                    assert all(W[k] % 256 == 0 for k in FIELDS), (n, nnz, T, P, L, Cn, O, R, H, W)
                    assert 0 == W["rows"] < W["tail"] <= W["thr"] < W["start"] < W["phase"] < W["cand"] < W["shifts"] < W["rec_ptr"] < W["rec"] < W["zeros"] \
                        < W["records"] < W["horizons"] < W["total"]
                    assert W["rec_ptr"] - W["shifts"] == al(Cn * 4)               # the sweep's regions end where the record tables begin
                    assert W["rec"] - W["rec_ptr"] == al((n + 1) * 4) and W["zeros"] - W["rec"] == al(R * 4)
                    assert W["records"] - W["zeros"] == al(O * 4) == W["horizons"] - W["records"] and W["total"] - W["horizons"] == al(H * 4)
                    assert W["tail"] == W["sweep_tail"]                           # the sweep's layout in front
                    # the sweep's own tail, unless the 64 bytes push the lists or the scan's state out of LDS: then it holds them
                    grown = W["thr"] - W["sweep_thr"]
                    lists_moved = _plan(lib, n, nb, 1000, False, 0)["lists_in_lds"] and not _plan(lib, n, nb, 1000, False, S)["lists_in_lds"]
                    state_moved = 2 * n <= 150 * 1024 < 2 * n + S
                    assert (grown > 0) == lists_moved, (n, grown)                  # (the lists' region already holds the scan's state)
                    assert W["rec_ptr"] == W["sweep_total"] + grown
                    if lists_moved:
                        assert W["thr"] - W["tail"] >= 1024 * 3 * n * 4
                    if state_moved:
                        assert W["thr"] - W["tail"] >= 2048 * 2 * n


def test_the_static_lds_is_counted_in_the_launch_plan(lib):
    S = lib.pst_static_lds()
    # lists in LDS: bitmaps + lists + counters within 48 KiB -- n = 11 232 without them, 11 216 with them
    assert 3 * (((11216 + 31) // 32 + 3) // 4 * 4) * 4 + 2 * 2 * 11216 + S <= 48 * 1024 < 3 * (((11217 + 31) // 32 + 3) // 4 * 4) * 4 + 2 * 2 * 11217 + S
    assert _plan(lib, 11232, 0, 1000, False, 0)["path"] == FRONTIER_LDS and _plan(lib, 11233, 0, 1000, False, 0)["path"] == FRONTIER_MEM
    assert _plan(lib, 11216, 0, 1000, False, S)["path"] == FRONTIER_LDS and _plan(lib, 11217, 0, 1000, False, S)["path"] == FRONTIER_MEM
    assert _plan(lib, 11217, 0, 1000, False, S)["grid"] <= 1024       # a workgroup per set of lists in the workspace
    # the scan's state in LDS: 2 n + counters within 150 KiB
    assert _plan(lib, 76800, 0, 1000, True, 0)["path"] == SCAN_LDS and _plan(lib, 76801, 0, 1000, True, 0)["path"] == SCAN_MEM
    assert _plan(lib, 76768, 0, 1000, True, S)["path"] == SCAN_LDS and _plan(lib, 76769, 0, 1000, True, S)["path"] == SCAN_MEM
    for n in (1, 34, 300, 4039, 4095, 4096, 9000, 20000, 70000, 200000):      # away from the boundaries: the same path and dynamic bytes
        for scan in (False, True):
            a, b = _plan(lib, n, 0, 10**6, scan, 0), _plan(lib, n, 0, 10**6, scan, S)
            assert (a["path"], a["lds"]) == (b["path"], b["lds"]) and b["grid"] <= a["grid"] and b["threads"] >= a["threads"], (n, scan, a, b)
            if b["path"] != SCAN_MEM:                                 # the workgroups of a CU and their counters fit its LDS
                assert -(-b["grid"] // 256) * (b["lds"] + S) <= 160 * 1024, (n, scan, b)


def _stage(lib, n, nnz, T, P, L, phase, W, G, init, Cn, shifts, rec, O, now, horizons, R=None, H=None, timed_bins=None):
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, t)            # noqa: E731
    phase, W, G, init, shifts = arr(phase, np.int32), arr(W, np.float64), arr(G, np.float64), arr(init, np.float64), arr(shifts, np.int32)
    hz = arr(horizons, np.int32)
    cols = [np.ascontiguousarray([r[j] for r in rec], np.int32) for j in range(4)]  # set, node, offset, kind
    R = len(rec) if R is None else R
    H = len(horizons) if H is None else H
    p = lambda a: None if a is None else a.ctypes.data                                # noqa: E731
    ptr, words = np.full(n + 1, -7, np.int32), np.zeros(max(R, 1), np.uint32)
    zeros, records, staged_h = np.zeros(max(O, 1), np.int32), np.zeros(max(O, 1), np.int32), np.full(max(H, 1), -7, np.int32)
    nr, nrec, nh = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    if timed_bins is not None:
        err = lib.pst_stage_timed(n, nnz, T, P, L, p(phase), p(W), p(G), p(init), Cn, p(shifts), *(p(c) for c in cols), R, O, timed_bins, p(ptr), p(words),
                                  p(zeros), p(records), C.byref(nr), C.byref(nrec)).decode()
    else:
        err = lib.pst_stage(n, nnz, T, P, L, p(phase), p(W), p(G), p(init), Cn, p(shifts), *(p(c) for c in cols), R, O, now, p(hz), H, p(ptr), p(words),
                            p(zeros), p(records), p(staged_h), C.byref(nr), C.byref(nrec), C.byref(nh)).decode()
    return err, nr.value, nrec.value, ptr, words, zeros, records, staged_h, nh.value


def test_staging_and_refusals(lib):
    n, nnz, T, P, L, Cn = 6, 8, 5, 3, 8, 4
    rng = np.random.default_rng(3)
    W, G = rng.uniform(0, 1, (P, nnz)), rng.uniform(0, 1, (P, n))
    phase = [7, 0, 2, 1, 2, 0, 1, 2]
    init = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.25, 0.25], [0.2, 0.8, 0.0], [1.0 / 3, 1.0 / 3, 1.0 / 3]])
    #      (set, node, offset, kind)
    rec = [(0, 4, 0, 1), (1, 2, -3, 3), (0, 4, -2, 0), (2, 0, 0, 0), (1, 4, -5, 4), (0, 1, -9, 0), (2, 0, 0, 0), (1, 5, -4, 2), (0, 4, 0, 1)]
    good = dict(n=n, nnz=nnz, T=T, P=P, L=L, phase=phase, W=W, G=G, init=init, Cn=Cn, shifts=[0, 3, 1, 3], rec=rec, O=3, now=2, horizons=[0, 1, 2])
    err, nr, nrec, ptr, words, zeros, records, hz, nh = _stage(lib, **good)
    assert (err, nr, nrec, nh) == ("", P * (nnz + n), len(rec) + n + 1 + 3 + 3, 3) and hz.tolist() == [0, 1, 2]
    assert ptr.tolist() == [0, 2, 3, 4, 4, 8, 9]                      # by node
    word = lambda s, v, d, k: s | k << 4 | min(-d, T) << 8            # noqa: E731  (back clamped to T: -9 and -5 both read 5)
    order = [3, 6, 5, 1, 0, 2, 4, 8, 7]                               # stable: a node's records in the order given
    assert words.tolist() == [word(*rec[i]) for i in order]
    assert zeros.tolist() == [2, 0, 2] and records.tolist() == [4, 3, 2]
    # equal to what sir_stage_timed stages, thresholds' count included: one record sort for both
    t = _stage(lib, **good, timed_bins=4)
    assert t[:3] == (err, nr, nrec) and all(np.array_equal(a, b) for a, b in zip(t[3:7], (ptr, words, zeros, records)))
    many = [(int(rng.integers(3)), int(rng.integers(n)), -int(rng.integers(0, 9)), int(rng.integers(5))) for _ in range(200)] + [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0)]
    a, b = _stage(lib, **dict(good, rec=many)), _stage(lib, **dict(good, rec=many), timed_bins=7)
    assert a[0] == "" == b[0] and all(np.array_equal(x, y) for x, y in zip(a[3:7], b[3:7]))
    # the edges of what is accepted
    assert _stage(lib, **dict(good, now=0, horizons=[4]))[0] == "" and _stage(lib, **dict(good, now=4, horizons=[0]))[0] == ""
    assert _stage(lib, **dict(good, now=0, horizons=[0, 1, 2, 3, 4], shifts=None))[0] == ""
    assert _stage(lib, **dict(good, T=1, L=8, now=0, horizons=[0], shifts=None))[0] == ""
    # no O * T limit: 16 sets at T = 2048, which sir_stage_timed refuses; 32 horizons
    long = dict(good, T=2048, L=2048, phase=[0] * 2048, shifts=None, O=16, rec=[(o, 1, 0, 0) for o in range(16)], now=1000, horizons=list(range(0, 64, 2)))
    err, _, _, _, _, _, records, hz, nh = _stage(lib, **long)
    assert err == "" and nh == 32 and hz.tolist() == list(range(0, 64, 2)) and records.tolist() == [1] * 16
    assert "2048" in _stage(lib, **long, timed_bins=4)[0]

    def refused(*where, **kw):
        err, nr, nrec, *_, nh = _stage(lib, **dict(good, **kw))
        assert err.startswith("entry: ") and all(w in err for w in where) and (nr, nrec, nh) == (0, 0, 0), (kw, err)

    refused("O = 0", O=0)
    refused("O = 17", O=17)
    refused("O = -1", O=-1)
    refused("now = -1", now=-1)
    refused("now = 5", "T = 5", now=5, horizons=[0])
    refused("now = 2048", **dict(long, now=2048, horizons=[0]))
    refused("H = 0", horizons=[], H=0)
    refused("H = 33", T=40, L=40, phase=[0] * 40, shifts=None, now=0, horizons=list(range(33)))
    refused("H = -1", H=-1)
    refused("horizons[0] = -1", horizons=[-1, 0, 1])
    refused("horizons[2] = 1", horizons=[0, 1, 1])
    refused("horizons[1] = 0", horizons=[1, 0])
    refused("horizons[2] = 3", "T - 1 = 4", horizons=[0, 1, 3])                   # now + 3 = 5 > T - 1
    refused("horizons[0] = 1", now=4, horizons=[1])
    refused("2^31", **dict(long, n=3_000_000, init=None, W=None, G=None, nnz=0))  # 16 x 32 x 2 x 3 000 000 cells; refused before anything is read
    refused("R = 0", R=0)
    refused("R = -1", R=-1)
    refused("rec_set[1] = 3", rec=[rec[0], (3, 2, -3, 3)] + rec[2:])
    refused("rec_set[4] = -1", rec=rec[:4] + [(-1, 4, -5, 4)] + rec[5:])
    refused("rec_node[2] = 6", rec=rec[:2] + [(0, 6, -2, 0)] + rec[3:])
    refused("rec_node[0] = -1", rec=[(0, -1, 0, 1)] + rec[1:])
    refused("rec_kind[7] = 5", rec=rec[:7] + [(1, 5, -4, 5)] + rec[8:])
    refused("rec_kind[3] = -1", rec=rec[:3] + [(2, 0, 0, -1)] + rec[4:])
    refused("rec_offset[8] = 1", rec=rec[:8] + [(0, 4, 1, 1)])
    refused("evidence set 1 holds no record", rec=[r for r in rec if r[0] != 1])
    refused("evidence set 3 holds no record", O=4)
    # the sweep's refusals, through the same function
    refused("shifts[2] = 4", shifts=[0, 3, 4, 9])
    refused("L = 4", "T = 5", L=4, phase=phase[:4], shifts=None)
    bad = list(phase); bad[6] = 3
    refused("phase[6] = 3", phase=bad)
    x = W.copy(); x[2, 7] = 1.5
    refused("phase 2", "position 7", W=x)
    x = init.copy(); x[3, 1] = -0.1
    refused("init[3][1]", init=x)
