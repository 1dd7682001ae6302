"""CPU: the exact Euler gradient's kept / persistent entry and its plan query (include/gnode.h, ABI 225) are exported, bound
and refuse bad calls before any pointer is touched; the kernels behind them declare no scratch.  No compute call is made."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from gnode.build import build_lib
    from gnode import _lib
    build_lib()
    return _lib.load()


def test_keep_entry_points_are_exported(lib):
    from gnode import _lib
    for name in ("gnode_backward_discrete_keep_f32", "gnode_backward_discrete_path"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert lib.gnode_version() >= 225
    assert len(_lib.ABI["gnode_backward_discrete_keep_f32"][1]) == len(_lib.ABI["gnode_backward_dx_f32"][1])


def _call(lib, keep=None, grads=None, gx=None, sol_info=-1):
    # (g, x, p, dt, n_steps, out_rows, n_out, sol, keep, keep_bytes, gS, gI, gR, grads, rows, H, ws, ws_bytes, stream, flags, sol_info, gx)
    return lib.gnode_backward_discrete_keep_f32(None, None, None, None, 0, None, 0, None, keep, 64 if keep else 0, None, None, None,
                                                grads, 1, 64, None, 0, None, 0, sol_info, gx)


def test_bad_calls_are_refused(lib):
    """neither grads nor gx; keep together with gx; keep with a trajectory that has no GNODE_SOL_KEEP (2); a keep-produced
    trajectory without its buffer; null pointers: all GNODE_ERR_ARG before any pointer is touched (16 stands for a pointer)"""
    from gnode import _lib
    grads = _lib.Params()                       # (gradient pointers travel in the same struct)
    import ctypes as C
    assert _call(lib) == ERR_ARG and b"neither" in lib.gnode_last_error()
    assert _call(lib, keep=16, gx=16, sol_info=2) == ERR_ARG and b"input gradient" in lib.gnode_last_error()
    assert _call(lib, keep=16, grads=C.byref(grads), sol_info=1) == ERR_ARG and b"filled none" in lib.gnode_last_error()
    assert _call(lib, grads=C.byref(grads), sol_info=2) == ERR_ARG and b"keep" in lib.gnode_last_error()
    assert _call(lib, keep=16, grads=C.byref(grads), sol_info=2) == ERR_ARG and b"null" in lib.gnode_last_error()
    assert _call(lib, grads=C.byref(grads), sol_info=1) == ERR_ARG and b"null" in lib.gnode_last_error()
    assert _call(lib, gx=16) == ERR_ARG and b"null" in lib.gnode_last_error()
    # the plan query answers -1 without a graph
    assert lib.gnode_backward_discrete_path(None, 100, 64, 10, None, 11, 1, 0, 2, 0) == -1


def test_old_entry_still_refuses_keep_trajectories(lib):
    st = lib.gnode_backward_discrete_f32(None, None, None, None, 0, None, 0, None, 2, None, None, None, None, 16, 1, 64,
                                         None, 0, None)
    assert st == ERR_ARG and b"keep" in lib.gnode_last_error()


def _resources(src):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), src], capture_output=True, text=True,
                         timeout=1500).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(\S.*?)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch\s+(\d+)", line)
        if m:
            rows[m.group(1).strip()] = tuple(int(v) for v in m.groups()[1:])
    return rows


def test_exact_sweeps_declare_no_scratch():
    """k_pers_bwd64<.., EXACT> and k_persg_bwd<.., EXACT>: no scratch, no vector spills, and no more vector registers than
    their adjoint twins (k_pers_bwd64 stays one workgroup of 256 NT threads per CU; k_persg_bwd fits its 256-register budget)"""
    r = _resources("gnode_pers64_bwd.hip")
    twins = [(k, k[:-len("true>")] + "false>") for k in r if k.startswith("k_pers_bwd64<") and k.endswith(", true>") and k.count(",") == 3]
    assert len(twins) == 8, sorted(r)
    for ex, ad in twins:
        assert r[ex][2] == 0 and r[ex][4] == 0, (ex, r[ex])
        assert r[ex][0] <= r[ad][0] <= 256, (ex, r[ex], r[ad])
    r = _resources("gnode_persg.hip")
    for lpr in (2, 4, 8):
        ex, ad = r[f"k_persg_bwd<{lpr}, true>"], r[f"k_persg_bwd<{lpr}, false>"]
        assert ex[2] == 0 and ex[4] == 0 and ex[0] <= ad[0] <= 256, (lpr, ex, ad)
