"""CPU: the host plan of the Monte-Carlo nowcast from evidence that may be wrong (sir_stage_strata in
csrc/gnode_sir_plan.cpp), off the GPU.  Like tests/test_sir_post_plan.py this module compiles the plan unit with the system g++,
here with that module's shim and tests/sir_strata_plan_shim.cpp, loads it with ctypes and checks that the staging is
sir_stage_post's for every accepted number of strata, that mismatches 0 to 7 are accepted and 8 and -1 refused, the cell limit O *
D * H * 2 * n < 2^31 at its exact boundary, and every refusal of the staging with the offending value in its message and nothing
staged.  (The workspace and the layout are the posterior's: tests/test_sir_post_plan.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gn-ode-sir_amd", "csrc")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("sirstrataplan")), "libsirstrataplan.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(CSRC, "gnode_sir_plan.cpp"), os.path.join(HERE, "sir_post_plan_shim.cpp"),
                    os.path.join(HERE, "sir_strata_plan_shim.cpp")], check=True)
    L = C.CDLL(so)
    vp, i64, i = C.c_void_p, C.c_int64, C.c_int
    p64 = C.POINTER(i64)
    L.pst_stage.restype, L.xst_stage.restype = C.c_char_p, C.c_char_p
    L.pst_stage.argtypes = [i, i64, i, i, i, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, vp, i, vp, vp, vp, vp, vp, p64, p64, p64]
    L.xst_stage.argtypes = [i, i64, i, i, i, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, vp, i, i, vp, vp, vp, vp, vp, p64, p64, p64]
    return L


def _stage(lib, n, nnz, T, P, L, phase, W, G, init, Cn, shifts, rec, O, now, horizons, M=None, R=None, H=None):
    """(error, thresholds staged, record entries staged, rec_ptr, rec, zeros, records, horizons, horizons staged) of
    sir_stage_strata, or of sir_stage_post for M = None"""
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
    front = (n, nnz, T, P, L, p(phase), p(W), p(G), p(init), Cn, p(shifts), *(p(c) for c in cols), R, O, now, p(hz), H)
    back = (p(ptr), p(words), p(zeros), p(records), p(staged_h), C.byref(nr), C.byref(nrec), C.byref(nh))
    err = (lib.pst_stage(*front, *back) if M is None else lib.xst_stage(*front, M, *back)).decode()
    return err, nr.value, nrec.value, ptr, words, zeros, records, staged_h, nh.value


def _good():
    n, nnz, T, P, L, Cn = 6, 8, 5, 3, 8, 4
    rng = np.random.default_rng(3)
    W, G = rng.uniform(0, 1, (P, nnz)), rng.uniform(0, 1, (P, n))
    phase = [7, 0, 2, 1, 2, 0, 1, 2]
    init = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.25, 0.25], [0.2, 0.8, 0.0], [1.0 / 3, 1.0 / 3, 1.0 / 3]])
    #      (set, node, offset, kind)
    rec = [(0, 4, 0, 1), (1, 2, -3, 3), (0, 4, -2, 0), (2, 0, 0, 0), (1, 4, -5, 4), (0, 1, -9, 0), (2, 0, 0, 0), (1, 5, -4, 2), (0, 4, 0, 1)]
    return dict(n=n, nnz=nnz, T=T, P=P, L=L, phase=phase, W=W, G=G, init=init, Cn=Cn, shifts=[0, 3, 1, 3], rec=rec, O=3, now=2, horizons=[0, 1, 2])


def _same(a, b):
    return a[:3] == b[:3] and a[8] == b[8] and all(np.array_equal(x, y) for x, y in zip(a[3:8], b[3:8]))


def test_the_strata_are_at_most_8(lib):
    assert lib.xst_maxd() == 8


def test_staging_is_the_posteriors_for_every_number_of_strata(lib):
    good = _good()
    post = _stage(lib, **good)
    assert post[0] == "" and post[2] > 0 and post[8] == 3
    for M in range(8):                                              # 0 .. GN_SIR_POST_MAXD - 1
        assert _same(_stage(lib, **good, M=M), post), M
    rng = np.random.default_rng(5)
    many = [(int(rng.integers(3)), int(rng.integers(6)), -int(rng.integers(0, 9)), int(rng.integers(5))) for _ in range(200)] + [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0)]
    assert _same(_stage(lib, **dict(good, rec=many), M=7), _stage(lib, **dict(good, rec=many)))
    long = dict(good, T=2048, L=2048, phase=[0] * 2048, shifts=None, O=16, rec=[(o, 1, 0, 0) for o in range(16)], now=1000, horizons=list(range(0, 64, 2)))
    assert _same(_stage(lib, **long, M=7), _stage(lib, **long)) and _stage(lib, **long)[0] == ""


def test_refusals_name_the_value_and_stage_nothing(lib):
    good = _good()
    rec, phase, W, init = good["rec"], good["phase"], good["W"], good["init"]

    def refused(*where, M=2, **kw):
        err, nr, nrec, *_, nh = _stage(lib, **dict(good, **kw), M=M)
        assert err.startswith("entry: ") and all(w in err for w in where) and (nr, nrec, nh) == (0, 0, 0), (kw, err)
        return err

    # the two of its own
    refused("mismatches = 8", "[0, 7]", M=8)
    refused("mismatches = -1", "[0, 7]", M=-1)
    refused("mismatches = 2147483647", M=2**31 - 1)
    # ... and the posterior's, with the posterior's words
    for kw, where in ((dict(O=0), "O = 0"), (dict(O=17), "O = 17"), (dict(now=-1), "now = -1"), (dict(now=5, horizons=[0]), "now = 5"),
                      (dict(horizons=[], H=0), "H = 0"), (dict(H=-1), "H = -1"), (dict(horizons=[-1, 0, 1]), "horizons[0] = -1"),
                      (dict(horizons=[0, 1, 1]), "horizons[2] = 1"), (dict(horizons=[0, 1, 3]), "horizons[2] = 3"), (dict(R=0), "R = 0"),
                      (dict(rec=[rec[0], (3, 2, -3, 3)] + rec[2:]), "rec_set[1] = 3"), (dict(rec=rec[:2] + [(0, 6, -2, 0)] + rec[3:]), "rec_node[2] = 6"),
                      (dict(rec=rec[:7] + [(1, 5, -4, 5)] + rec[8:]), "rec_kind[7] = 5"), (dict(rec=rec[:8] + [(0, 4, 1, 1)]), "rec_offset[8] = 1"),
                      (dict(rec=[r for r in rec if r[0] != 1]), "evidence set 1 holds no record"), (dict(shifts=[0, 3, 4, 9]), "shifts[2] = 4"),
                      (dict(L=4, phase=phase[:4], shifts=None), "L = 4")):
        assert refused(where, **kw) == _stage(lib, **dict(good, **kw))[0], kw
    refused("H = 33", T=40, L=40, phase=[0] * 40, shifts=None, now=0, horizons=list(range(33)))
    bad = list(phase); bad[6] = 3
    refused("phase[6] = 3", phase=bad)
    x = W.copy(); x[2, 7] = 1.5
    refused("phase 2", "position 7", W=x)
    x = init.copy(); x[3, 1] = -0.1
    refused("init[3][1]", init=x)
    # mismatches is judged first: a bad M with a bad `now` names M
    refused("mismatches = 9", M=9, now=-1)


def test_the_cell_limit_at_its_exact_boundary(lib):
    """O * D * H * 2 * n < 2^31 with O = 16, H = 32: D = 8 admits n = 262 143 and refuses 262 144, which D = 7 admits; the
    posterior's own limit (D = 1) lies at n = 2 097 152"""
    T, H = 40, 32
    assert 16 * 8 * H * 2 * 262143 < 2**31 == 16 * 8 * H * 2 * 262144 and 16 * 7 * H * 2 * 262144 < 2**31 == 16 * H * 2 * 2097152

    def at(n, M):
        init = np.tile([1.0, 0.0, 0.0], (n, 1))
        return _stage(lib, n=n, nnz=0, T=T, P=1, L=T, phase=[0] * T, W=None, G=np.full((1, n), 0.5), init=init, Cn=2, shifts=None,
                      rec=[(o, n - 1 - o, 0, o % 5) for o in range(16)], O=16, now=3, horizons=list(range(H)), M=M)

    ok = at(262143, 7)
    assert ok[0] == "" and ok[1] == 262143 and ok[8] == H and ok[6].tolist() == [1] * 16 and int(ok[3][-1]) == 16
    err, nr, nrec, *_, nh = at(262144, 7)
    assert err.startswith("entry: ") and all(w in err for w in ("O = 16", "D = 8", "H = 32", "n = 262144", "2^31")) and (nr, nrec, nh) == (0, 0, 0), err
    assert at(262144, 6)[0] == "" and at(262144, 0)[0] == ""
    err = at(2097152, 0)[0]                                         # the posterior's own refusal comes first, in its words
    assert "2^31" in err and "D =" not in err
    assert at(2097151, 0)[0] == "" and "D = 2" in at(2097151, 1)[0]
