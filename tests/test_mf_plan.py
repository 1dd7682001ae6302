"""CPU: the host-only unit of the mean-field's reverse sweep (csrc/gnode_mf_plan.cpp), compiled with the system g++ together with
tests/mf_plan_shim.cpp and loaded with ctypes, as tests/test_graph_plan.py does for the graph plan: which step lists it
accepts, the per-interval maximum it returns, every refusal with its interval named, and the workspace layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import meanfield_grad_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gn-ode-sir_amd", "csrc")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("mfplan")), "libmfplan.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(CSRC, "gnode_mf_plan.cpp"), os.path.join(HERE, "mf_plan_shim.cpp")], check=True)
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.mp_check.restype, lib.mp_check.argtypes = C.c_int, [vp, C.c_int32, vp, C.c_int64, vp, C.POINTER(C.c_int32), C.c_char_p, C.c_int]
    lib.mp_layout.restype, lib.mp_layout.argtypes = None, [C.c_int64, C.c_int64, C.c_int32, vp]
    return lib


def check(lib, t_out, h, n_acc, n_h=None):
    """(max_interval_steps, "") or (None, message)"""
    t_out, h, n_acc = np.ascontiguousarray(t_out, np.float64), np.ascontiguousarray(h, np.float64), np.ascontiguousarray(n_acc, np.int32)
    mx, err = C.c_int32(-1), C.create_string_buffer(512)
    rc = lib.mp_check(t_out.ctypes.data, len(t_out), h.ctypes.data, len(h) if n_h is None else n_h, n_acc.ctypes.data, C.byref(mx), err, 512)
    return (mx.value, "") if rc == 0 else (None, err.value.decode())


def walk(t_out, parts):
    """a valid list: interval `to` takes parts[to - 1] (numbers in (0, 1) that add up to less than 1) of its length as the
    steps before the last, and the last step is what the forward's clipping leaves, t_end - t"""
    h, n_acc = [], [0]
    for to in range(1, len(t_out)):
        t, t_end = t_out[to - 1], t_out[to]
        if t_end == t:
            n_acc.append(0)
            continue
        for f in parts[to - 1]:
            h.append(f * (t_end - t_out[to - 1]))
            t = t + h[-1]
        h.append(t_end - t)
        n_acc.append(len(parts[to - 1]) + 1)
    return np.array(h), np.array(n_acc, np.int32)


T_OUT = np.array([0.0, 1.0, 1.0, 2.5, 2.5, 2.5, 7.0])
PARTS = [[0.1, 0.3], [], [0.2], [], [], [0.01, 0.05, 0.2, 0.3, 0.3]]


def test_valid_lists_are_accepted(lib):
    h, n_acc = walk(T_OUT, PARTS)
    assert list(n_acc) == [0, 3, 0, 2, 0, 0, 6]
    assert check(lib, T_OUT, h, n_acc) == (6, "")
    assert check(lib, [0.0], [], [0]) == (0, "")                                   # n_out = 1
    assert check(lib, [0.0, 0.0, 0.0], [], [0, 0, 0]) == (0, "")                   # only repeated times
    assert check(lib, [0.0, 3.0], [3.0], [0, 1]) == (1, "")                        # one step, exactly the interval
    t_out = M._times(1, 8)                                                         # what the model's controller records
    rp, ci = M.random_graph(20, 40, 1)
    c = M._inputs(rp, ci, 1, 2)
    _, hh, acc, _ = M.dp5_adaptive(rp, ci, c["init"], c["beta"], c["gamma"], c["w"], t_out, 1e-6, 1e-8)
    assert check(lib, t_out, hh, acc) == (int(acc.max()), "")


def _refused(lib, t_out, h, n_acc, interval, n_h=None):
    mx, msg = check(lib, t_out, h, n_acc, n_h)
    assert mx is None and msg.startswith(f"mp_check: step list, interval {interval}: "), msg
    return msg


def test_refusals_name_the_interval(lib):
    h, n_acc = walk(T_OUT, PARTS)
    for bad in (0.0, -0.25, float("nan"), float("inf")):                           # a step that is not finite and > 0
        for at, interval in ((1, 1), (3, 3), (7, 6)):
            x = h.copy()
            x[at] = bad
            assert "not a finite step > 0" in _refused(lib, T_OUT, x, n_acc, interval)
    last = {1: 2, 3: 4, 6: 10}                                                     # interval -> the position of its last step
    for interval, at in last.items():
        for other in (np.nextafter(h[at], np.inf), np.nextafter(h[at], -np.inf)):  # over and short by one ulp
            x = h.copy()
            x[at] = other
            assert "the last step" in _refused(lib, T_OUT, x, n_acc, interval)
    x = h.copy()
    x[0] = 2.0                                                                     # a step before the last that reaches t_end
    assert "before the last" in _refused(lib, T_OUT, x, n_acc, 1)
    acc = n_acc.copy()
    acc[3] = 0                                                                     # a positive interval without a step ...
    assert "no step from t=1 to t=2.5" in _refused(lib, T_OUT, h[[0, 1, 2, 5, 6, 7, 8, 9, 10]], acc, 3)
    acc = n_acc.copy()
    acc[2] = 1                                                                     # ... and steps in an interval of no length
    assert _refused(lib, T_OUT, np.insert(h, 3, 0.5), acc, 2)
    assert "add up to 11 steps, the list has 12" in _refused(lib, T_OUT, np.append(h, 0.5), n_acc, 6)      # count mismatches
    assert "run past the list" in _refused(lib, T_OUT, h, n_acc, 6, n_h=10)
    acc = n_acc.copy()
    acc[0] = 1
    assert _refused(lib, T_OUT, h, acc, 0)
    acc = n_acc.copy()
    acc[1] = -1
    assert "negative" in _refused(lib, T_OUT, h, acc, 1)


def test_layout(lib):
    for rows, nnz, m in ((1, 0, 0), (257, 1400, 13), (900, 1798, 110), (4039 * 16, 176468, 40)):
        o = np.zeros(8, np.uint64)
        lib.mp_layout(rows, nnz, m, o.ctypes.data)
        o = [int(x) for x in o]
        assert all(x % 256 == 0 for x in o) and o[0] == 0
        sizes = [3 * rows * 8, 5 * -(-3 * rows * 8 // 256) * 256, 18 * rows * 8, 12 * rows * 8, 2 * -(-rows * 8 // 256) * 256, max(nnz, 1) * 8,
                 (m + 1) * -(-3 * rows * 8 // 256) * 256]
        for k in range(7):                                                         # each array fits in front of the next
            assert o[k] + sizes[k] <= o[k + 1], k
        assert o[7] <= sum(-(-s // 256) * 256 for s in sizes)                      # and nothing else is asked for
