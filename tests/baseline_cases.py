"""The DMP baseline's cases for the GPU tests (a helper, not a test): graphs, per-edge weights that are not symmetric in value,
per-node gamma, seeds and horizons (numpy only), the bars they are held to, and the model under test built from a case.
tests/test_gpu_baselines.py says what each case is for."""
import functools
import hashlib
import json
import os

import numpy as np

RTOL = 1e-5                     # test_gpu_parity.py's fp32 bar
MF_ATOL = 1e-6                  # the project's mean-field bar


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30)


def f32_digest(a):
    """SHA-256 of the contiguous bytes of a float32 array or tensor: what tests/golden/dmp_parent.json holds per output."""
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    assert a.dtype == np.float32
    return hashlib.sha256(a.tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def dmp_parent():
    """{key: entry} of tests/golden/dmp_parent.json (make_golden_dmp_parent.py says what the keys are)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dmp_parent.json")) as f:
        return {e["key"]: e for e in json.load(f)["entries"]}


def is_parents(key, out):
    """`out` has the shape and the bits that the parent library returned for the call `key`."""
    e = dmp_parent()[key]
    return list(out.shape) == e["shape"] and f32_digest(out) == e["sha256"]


def candidates_entry(out, **sizes):
    """What tests/golden/dmp_candidates_parent.json holds for one call of a candidate sweep: the shape of its float64 output, the
    SHA-256 of its bytes, and the sizes and the tile that the library answered for the call's graph.  Finite, or nothing to hash."""
    a = np.ascontiguousarray(out.cpu().numpy())
    assert a.dtype == np.float64 and np.isfinite(a).all()
    return {"shape": list(a.shape), "sha256": hashlib.sha256(a.tobytes()).hexdigest(), **{k: int(v) for k, v in sizes.items()}}


@functools.lru_cache(maxsize=None)
def dmp_candidates_parent():
    """{key: entry} of tests/golden/dmp_candidates_parent.json (make_golden_dmp_candidates_parent.py says what the keys are)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dmp_candidates_parent.json")) as f:
        return json.load(f)["entries"]


def assert_candidates_parents(entries):
    """every (key, entry) that a module's `parent_entries` recomputed is the fixture's: shape, bits, sizes and tile"""
    for key, got in entries:
        assert got == dmp_candidates_parent()[key], key


def schedule_entry(tensors, workspace_bytes, one_workgroup):
    """What tests/golden/dmp_schedule_parent.json holds for one scheduled call: per float32 output (None: not returned, a table
    without entries) its shape and the SHA-256 of its bytes, the workspace the library asked for and whether the one-workgroup
    form served the graph.  Every output is finite and not all zeros, or there is nothing to hash."""
    shapes, digests = [], []
    for t in tensors:
        if t is None:
            shapes.append(None); digests.append(None)
            continue
        a = np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t)
        assert a.dtype == np.float32 and np.isfinite(a).all() and a.any()
        shapes.append(list(a.shape)); digests.append(hashlib.sha256(a.tobytes()).hexdigest())
    return {"shape": shapes, "sha256": digests, "workspace_bytes": int(workspace_bytes), "one_workgroup": bool(one_workgroup)}


@functools.lru_cache(maxsize=None)
def dmp_schedule_parent():
    """{key: entry} of tests/golden/dmp_schedule_parent.json (make_golden_dmp_schedule_parent.py says what the keys are); each
    direction holds an entry of each form."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dmp_schedule_parent.json")) as f:
        entries = json.load(f)["entries"]
    for direction in ("forward/", "backward/"):
        assert {e["one_workgroup"] for k, e in entries.items() if k.startswith(direction)} == {True, False}, direction
    return entries


def assert_schedule_parents(entries):
    """every (key, entry) that a module's `parent_entries` recomputed is the fixture's: shapes, bits, workspace and form"""
    for key, got in entries:
        assert got == dmp_schedule_parent()[key], key


def weights(nnz, lo, hi, seed):
    return np.random.default_rng(seed).uniform(lo, hi, size=nnz).astype(np.float32)   # per directed edge: w_uv != w_vu


def gammas(n, seed):
    return np.random.default_rng(seed).uniform(0.1, 0.5, size=n).astype(np.float32)


def er(n, m, seed):
    import gnode_oracle as O
    rp, ci, e = O.er_graph(n, m, seed=seed)
    return rp, ci, e


def _case(rp, ci, w, gam, seeds, T):
    return dict(rp=rp, ci=ci, w=w, gam=gam, seeds=[int(s) for s in seeds], T=int(T))


def _case_hub():
    import gnode_oracle as O
    rp, ci, _ = O.chung_lu_graph(3001, 40000, seed=2)
    return _case(rp, ci, weights(len(ci), 0.02, 0.3, 5), gammas(3001, 6), [0, 17, 2500], 10)


def _case_isolated():
    rp, ci, _ = er(513, 40, 6)
    deg = np.diff(rp)
    iso, con = int(np.flatnonzero(deg == 0)[0]), int(np.flatnonzero(deg > 0)[0])
    return _case(rp, ci, weights(len(ci), 0.05, 0.5, 7), gammas(513, 8), [iso, con], 7)


def _case_horizon(T):
    rp, ci, _ = er(300, 900, 7)
    return _case(rp, ci, weights(len(ci), 0.05, 0.4, 9), gammas(300, 10), [5, 250], T)


def _case_nnz0():
    return _case(np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), gammas(5, 11), [1, 3], 6)


def _case_seeds(seeds):
    rp, ci, _ = er(400, 1200, 8)
    return _case(rp, ci, weights(len(ci), 0.05, 0.4, 12), gammas(400, 13), seeds, 8)


def _case_w_one():
    rp, ci, e = er(34, 78, 3)
    return _case(rp, ci, np.ones(len(ci), np.float32), gammas(34, 14), e[0], 3)       # e[0]: two adjacent seeds


def _case_w_zero():
    rp, ci, _ = er(34, 78, 3)
    w = weights(len(ci), 0.05, 0.6, 15)
    w[::3] = 0.0                                                    # a third of the directed edges never transmit
    return _case(rp, ci, w, gammas(34, 16), [0, 20], 12)


def _case_gamma_01():
    rp, ci, _ = er(34, 78, 3)
    gam = gammas(34, 17)
    gam[0::3] = 0.0                                                 # never recover (seed 0 among them)
    gam[1::3] = 1.0                                                 # recover within the step (seed 1 among them)
    return _case(rp, ci, weights(len(ci), 0.05, 0.6, 18), gam, [0, 1, 20], 12)


DMP_CASES = {
    "hub": _case_hub, "isolated": _case_isolated, "T2": lambda: _case_horizon(2), "T3": lambda: _case_horizon(3),
    "nnz0": _case_nnz0, "seeds_none": lambda: _case_seeds([]), "seeds_all": lambda: _case_seeds(range(400)),
    "w_one": _case_w_one, "w_zero": _case_w_zero, "gamma_01": _case_gamma_01,
}


def dmp_model(c):
    import scipy.sparse as sp
    from gnode.dmp import DMP_SIR
    n = len(c["rp"]) - 1
    return DMP_SIR(sp.csr_matrix((c["w"], c["ci"], c["rp"]), shape=(n, n)), c["gam"])
