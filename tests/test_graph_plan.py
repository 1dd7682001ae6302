"""CPU: the graph handle's plan (csrc/gnode_graph_plan.cpp) is pinned off the GPU.

The plan unit is plain C++; this module compiles it with the system g++ together with tests/graph_plan_shim.cpp, loads the
object with ctypes and checks
  * that every array the handle uploads, every scalar it keeps and every per-call plan (k_pers64, its adjoint sweep, k_persg)
    is the one tests/golden/graph_plan_parent.json recorded from the commit before the plan unit existed (SHA-256 of the
    arrays' little-endian bytes; the recipe is in the fixture's "recipe" entry), and
  * the invariants the kernels rely on, recomputed in numpy from the CSR alone, and
  * the edge tables src, rev and `symmetric` (younger than that fixture, so read through shim functions of their own): the
    identities that define them, tests/dmp_grad_model.py's restatement, the small graphs at which a search or an expansion goes
    wrong, an asymmetric pattern; the unit runs once under AddressSanitizer and UBSan in a program of its own.
The argument checks of gnode_graph_create (which sit in front of any HIP call) go through the hipcc-built library."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import fixture_cases as FC

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gn-ode-sir_amd", "csrc")
FIXTURE = os.path.join(HERE, "golden", "graph_plan_parent.json")

BATCHES, STEPS, CUS, HIDDEN = (1, 2, 4, 8, 9, 64, 65), (1, 2, 59, 127, 128, 129), (256, 64, 60), (8, 16, 32)
ARRAYS = ["rowhdr", "hubidx", "seg_lo", "seg_hi", "hub_seg_ptr", "pgmap"] + [f"{a}{16 << i}" for i in range(3) for a in ("persmap", "pershub", "perssegptr", "perssegitem")]
N_SCALARS = 49


# --------------------------------------------------------------------------- the graphs
def _csr(n, u, v):
    """symmetrised CSR (sorted columns, no duplicates, no self-loops) of the undirected edges (u, v)"""
    import scipy.sparse as sp
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    A = sp.coo_matrix((np.ones(2 * u.shape[0], np.int8), (np.concatenate([u, v]), np.concatenate([v, u]))), shape=(n, n)).tocsr()
    A.setdiag(0)
    A.eliminate_zeros()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32)


def _star_on_er(n, m, seed, hub_edges):
    """sparse G(n, m) in which node 0 is joined to nodes 1 .. hub_edges as well"""
    rp, ci = FC.synth().er_csr(n, m, seed)
    rows = np.repeat(np.arange(n), np.diff(rp))
    return _csr(n, np.concatenate([rows, np.zeros(hub_edges, np.int64)]), np.concatenate([ci, np.arange(1, hub_edges + 1)]))


def _graphs():
    import networkx as nx
    sy = FC.synth()
    out = {}
    names = [str(s) for s in np.load(os.path.join(FC.GOLDEN, "real_graphs.npz"))["names"]]
    for name, (rp, ci) in zip(names, FC.graphs()):
        out["real_" + name] = (rp.astype(np.int32), ci.astype(np.int32))
    e = np.array(nx.karate_club_graph().edges())
    out["karate"] = _csr(34, e[:, 0], e[:, 1])
    out["er1893"] = sy.er_csr(1893, 13835, 0)
    out["heavy2000"] = sy.heavy_tail_csr(2000, 16000, seed=1)
    out["single_node"] = (np.zeros(2, np.int32), np.zeros(0, np.int32))
    for n in (16384, 16385, 32768, 32769):                 # either side of the k_pers64 and the k_persg resident-grid bounds
        out[f"er{n}"] = sy.er_csr(n, 2 * n, 7)
    out["hubs200"] = sy.er_csr(200, 12000, 3)              # mean degree 120: more than half the lane-group slots would be hubs
    out["bighub5000"] = _star_on_er(5000, 10000, 5, 4200)  # 132 segments in one workgroup: more than the 128 partial slots
    out["hub3980"] = _star_on_er(5000, 175000, 5, 3980)    # 125 segments fit the slots, but not 16 lane groups' item lists
    return out


@pytest.fixture(scope="module")
def graphs():
    return _graphs()


# --------------------------------------------------------------------------- the plan unit behind ctypes
def build_shim(tmp):
    so = os.path.join(str(tmp), "libgraphplan.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                    os.path.join(CSRC, "gnode_graph_plan.cpp"), os.path.join(HERE, "graph_plan_shim.cpp")], check=True)
    return load_shim(so)


def load_shim(so):
    lib = C.CDLL(so)
    vp, i32, i64, lng = C.c_void_p, C.c_int32, C.c_int64, C.c_long
    lib.gp_plan.restype, lib.gp_plan.argtypes = vp, [vp, vp, i32, i64]
    lib.gp_error.restype, lib.gp_error.argtypes = C.c_char_p, [vp]
    lib.gp_free.restype, lib.gp_free.argtypes = None, [vp]
    lib.gp_scalars.restype, lib.gp_scalars.argtypes = None, [vp, vp]
    lib.gp_array.restype, lib.gp_array.argtypes = vp, [vp, C.c_int, C.POINTER(i64)]
    lib.gp_edge_table.restype, lib.gp_edge_table.argtypes = vp, [vp, C.c_int, C.POINTER(i64)]
    lib.gp_symmetric.restype, lib.gp_symmetric.argtypes = C.c_int, [vp]
    lib.gp_pers64_plan.restype, lib.gp_pers64_plan.argtypes = C.c_int, [vp, C.c_int, lng, C.c_int, vp]
    lib.gp_pers_bwd64_plan.restype, lib.gp_pers_bwd64_plan.argtypes = C.c_int, [vp, C.c_int, lng, C.c_int, vp]
    lib.gp_persg_plan.restype, lib.gp_persg_plan.argtypes = C.c_int, [vp, C.c_int, lng, C.c_int, C.c_int, vp]
    lib.gp_const.restype, lib.gp_const.argtypes = C.c_int, [C.c_int]
    return lib


class Plan:
    """one graph's plan: scalars by name, arrays as numpy copies (None: not uploaded), the per-call planners"""

    def __init__(self, lib, rp, ci):
        self.lib, self.rp, self.ci, self.n = lib, np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32), rp.shape[0] - 1
        self.h = lib.gp_plan(self.rp.ctypes.data, self.ci.ctypes.data, self.n, int(self.rp[-1]))
        self.error = lib.gp_error(self.h).decode()
        if self.error:
            return
        s = np.zeros(N_SCALARS, np.int32)
        lib.gp_scalars(self.h, s.ctypes.data)
        s = [int(v) for v in s]
        self.scalars = {"max_degree": s[0], "n_bigrow": s[1], "n_hub": s[2], "n_seg": s[3], "pers_present": s[4:7], "perslds": s[7:10],
                        "persitems": s[10:13], "pgoff": s[13:25], "pgids": s[25:37], "pgsegs": s[37:49]}
        self.arrays = {}
        for k, name in enumerate(ARRAYS):
            ln = C.c_int64(0)
            p = lib.gp_array(self.h, k, C.byref(ln))
            self.arrays[name] = None if ln.value < 0 else np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), (ln.value,)).copy() if ln.value else np.zeros(0, np.int32)
        self.src, self.rev = (self._edge_table(k) for k in range(2))   # apart from ARRAYS: the parent's fixture has no entry for them
        self.symmetric = bool(lib.gp_symmetric(self.h))

    def _edge_table(self, which):
        ln = C.c_int64(0)
        p = self.lib.gp_edge_table(self.h, which, C.byref(ln))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), (ln.value,)).copy() if ln.value else np.zeros(0, np.int32)

    def close(self):
        self.lib.gp_free(self.h)

    def planner_table(self, which, num_cu):
        """[len(BATCHES) * len(STEPS)][1 + fields] int64: found, then the plan's fields (0 when there is no plan)"""
        rows = []
        for B in BATCHES:
            for T in STEPS:
                if which.startswith("persg"):
                    o = np.zeros(7, np.int64)
                    ok = self.lib.gp_persg_plan(self.h, num_cu, B * self.n, int(which[5:]), T, o.ctypes.data)
                else:
                    o = np.zeros(10, np.int32)
                    ok = getattr(self.lib, f"gp_{which}_plan")(self.h, num_cu, B, T, o.ctypes.data)
                rows.append([ok] + [int(v) for v in o] if ok else [0] * (1 + o.shape[0]))
        return np.array(rows, np.int64)


PLANNERS = ["pers64", "pers_bwd64"] + [f"persg{H}" for H in HIDDEN]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).astype("<i4" if a.dtype == np.int32 else "<i8").tobytes()).hexdigest()


def record(lib, graphs):
    """what the fixture holds per graph: scalars, array digests, and per planner and CU count the digest of its table and
    how many of its (batch, steps) cells have a plan"""
    out = {}
    for name, (rp, ci) in graphs.items():
        p = Plan(lib, rp, ci)
        assert not p.error, (name, p.error)
        out[name] = {"n": p.n, "nnz": int(rp[-1]), "scalars": p.scalars,
                     "arrays": {k: None if a is None else {"len": int(a.shape[0]), "sha256": _sha(a)} for k, a in p.arrays.items()},
                     "planners": {w: {str(cu): (lambda t: {"plans": int(t[:, 0].sum()), "sha256": _sha(t)})(p.planner_table(w, cu)) for cu in CUS}
                                  for w in PLANNERS}}
        p.close()
    return out


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("graphplan"))


@pytest.fixture(scope="module")
def parent():
    return json.load(open(FIXTURE))


# --------------------------------------------------------------------------- the plan is the parent's
def test_fixture_covers_every_branch(parent, graphs):
    """the recorded plans really take the branches the graphs were chosen for (checked on the parent while recording)"""
    g = parent["graphs"]
    assert set(g) == set(graphs)
    sc = {k: v["scalars"] for k, v in g.items()}
    assert sc["real_wiki-vote"]["n_hub"] == 568 and sc["real_fb-social"]["n_hub"] > 0
    assert sc["er16384"]["pers_present"] == [1, 1, 1] and sc["er16385"]["pers_present"] == [0, 0, 0]              # kPersMaxRows
    assert max(sc["er32768"]["pgoff"]) >= 0 and max(sc["er32769"]["pgoff"]) == -1 and g["er32769"]["arrays"]["pgmap"]["len"] == 0
    assert sc["hubs200"]["n_hub"] > 100 and sc["hubs200"]["pers_present"] == [0, 0, 0]                              # half the slots hubs
    assert sc["bighub5000"]["max_degree"] >= 4200 and sc["bighub5000"]["pers_present"] == [0, 0, 0]                 # 132 > PERS_MAX_PARTIALS in every variant
    assert sc["hub3980"]["pers_present"] == parent["hub3980_survivors"] and 0 < sum(sc["hub3980"]["pers_present"]) < 3   # PERS_MAX_ITEMS
    assert sc["single_node"]["pers_present"] == [1, 1, 1] and g["single_node"]["arrays"]["perssegitem16"]["len"] == 0
    for k in ("karate", "er1893"):
        assert sc[k]["n_hub"] == 0 and g[k]["arrays"]["hubidx"]["len"] == 0                                         # hub arrays not uploaded
    for k, v in g.items():                                                                                          # some plan and some refusal everywhere it can matter
        cells = len(BATCHES) * len(STEPS)
        assert all(0 <= c["plans"] <= cells for w in v["planners"].values() for c in w.values())
    assert g["real_fb-social"]["planners"]["pers64"]["256"]["plans"] > 0 and g["real_fb-social"]["planners"]["pers64"]["60"]["plans"] == 0
    assert g["real_fb-social"]["planners"]["pers_bwd64"]["256"]["plans"] > 0 and g["karate"]["planners"]["persg8"]["64"]["plans"] > 0


def test_plan_equals_parent(lib, parent, graphs):
    now = record(lib, graphs)
    for name, want in parent["graphs"].items():
        got = now[name]
        assert got["scalars"] == want["scalars"], name
        assert (got["n"], got["nnz"]) == (want["n"], want["nnz"]), name
        for k in ARRAYS:
            assert got["arrays"][k] == want["arrays"][k], (name, k)
        for w in PLANNERS:
            assert got["planners"][w] == want["planners"][w], (name, w)


# --------------------------------------------------------------------------- what the kernels rely on, from the CSR alone
def _check_pers64(p, i, hub_t, seg, max_items, max_partials):
    rp, n = p.rp.astype(np.int64), p.n
    deg = np.diff(rp)
    per_wg = 16 << i
    wgs = (n + per_wg - 1) // per_wg
    m, hub, segptr, items = (p.arrays[f"{a}{per_wg}"] for a in ("persmap", "pershub", "perssegptr", "perssegitem"))
    assert m.shape[0] == wgs * per_wg and hub.shape[0] == segptr.shape[0] == 2 * m.shape[0] and items.shape[0] % 4 == 0
    assert np.array_equal(np.sort(m[m >= 0]), np.arange(n)) and np.all(m[m < 0] == -1)          # every node once, padding -1
    hub, segptr, items = hub.reshape(-1, 2), segptr.reshape(-1, 2), items.reshape(-1, 4)
    is_hub = (m >= 0) & (deg[np.maximum(m, 0)] > hub_t)
    assert np.all(hub[~is_hub] == [-1, 0])
    assert np.array_equal(hub[is_hub, 1], (deg[m[is_hub]] + seg - 1) // seg)
    # lane groups' item lists follow one another in slot order and cover `items` exactly
    assert np.array_equal(segptr[:, 0], np.concatenate([[0], np.cumsum(segptr[:, 1])[:-1]])) and segptr[:, 1].sum() == items.shape[0]
    assert segptr[:, 1].max(initial=0) <= max_items and p.scalars["persitems"][i] == segptr[:, 1].max(initial=0)
    assert np.all(items[:, 3] == 0) and np.all(items[:, 1] - items[:, 0] <= seg) and np.all(items[:, 1] > items[:, 0])
    lds = 0
    for wg in np.flatnonzero(is_hub.reshape(wgs, per_wg).any(axis=1)) if items.shape[0] else []:
        sl = slice(wg * per_wg, (wg + 1) * per_wg)
        it = items[segptr[sl][0, 0]:segptr[sl][-1, 0] + segptr[sl][-1, 1]]
        it = it[np.argsort(it[:, 2], kind="stable")]
        assert np.array_equal(it[:, 2], np.arange(it.shape[0]))                                 # each partial slot of the workgroup once
        want = []
        for s in np.flatnonzero(is_hub[sl]):                                                    # a hub's slots: consecutive, in segment order,
            r, first = m[sl][s], hub[sl][s, 0]                                                  # tiling its CSR range in <= 32-edge pieces
            assert first == len(want)
            want += [(e, min(rp[r + 1], e + seg)) for e in range(rp[r], rp[r + 1], seg)]
        assert [tuple(x) for x in it[:, :2]] == want
        lds = max(lds, it.shape[0])
    no_items = segptr.reshape(wgs, per_wg, 2)[~is_hub.reshape(wgs, per_wg).any(axis=1)]
    assert np.all(no_items[:, :, 1] == 0)
    assert lds <= max_partials and p.scalars["perslds"][i] == lds


def _check_persg(p, hub_t, seg):
    n, deg = p.n, np.diff(p.rp.astype(np.int64))
    off = 0
    for vi in range(3):
        for nw in range(1, 5):
            k = vi * 4 + nw - 1
            gpw = (32 >> vi) * nw
            wps = (n + gpw - 1) // gpw
            if p.scalars["pgoff"][k] < 0:
                assert wps > 256 and p.scalars["pgids"][k] == p.scalars["pgsegs"][k] == 0
                continue
            assert p.scalars["pgoff"][k] == off                                                 # the variants tile the one allocation
            m = p.arrays["pgmap"][off:off + wps * gpw]
            off += wps * gpw
            assert np.array_equal(np.sort(m[m >= 0]), np.arange(n)) and np.all(m[m < 0] == -1)
            d = np.where(m >= 0, deg[np.maximum(m, 0)], 0).reshape(wps, gpw)
            hubrow = (d > hub_t) & (p.scalars["n_hub"] > 0)
            assert p.scalars["pgids"][k] == np.where(hubrow, 0, d).sum(axis=1).max()
            assert p.scalars["pgsegs"][k] == np.where(hubrow, (d + seg - 1) // seg, 0).sum(axis=1).max()
    assert off == p.arrays["pgmap"].shape[0]


def test_plan_invariants(lib, graphs):
    hub_t, seg, max_items, max_partials, max_rows, bigrow = (lib.gp_const(k) for k in range(6))
    assert (hub_t, seg, max_items, max_partials, max_rows, bigrow) == (96, 32, 8, 128, 16384, 512)
    for name, (rp, ci) in graphs.items():
        p = Plan(lib, rp, ci)
        n, deg = p.n, np.diff(rp.astype(np.int64))
        assert p.scalars["max_degree"] == deg.max() and p.scalars["n_bigrow"] == (deg > bigrow).sum(), name
        hdr = p.arrays["rowhdr"].reshape(n, 20)
        assert np.array_equal(hdr[:, 0], rp[:-1]) and np.array_equal(hdr[:, 1], rp[1:]) and np.all(hdr[:, 2:4] == 0), name
        first = np.zeros((n, 16), np.int32)
        for k in range(16):
            has = deg > k
            first[has, k] = ci[rp[:-1][has] + k]
        assert np.array_equal(hdr[:, 4:], first), name
        hubs = np.flatnonzero(deg > hub_t)
        assert p.scalars["n_hub"] == hubs.shape[0], name
        if hubs.shape[0]:
            want = np.full(n, -1, np.int32)
            want[hubs] = np.arange(hubs.shape[0])
            lo = np.concatenate([np.arange(rp[r], rp[r + 1], seg) for r in hubs])
            hi = np.concatenate([np.minimum(np.arange(rp[r], rp[r + 1], seg) + seg, rp[r + 1]) for r in hubs])
            ptr = np.concatenate([[0], np.cumsum((deg[hubs] + seg - 1) // seg)])
            assert np.array_equal(p.arrays["hubidx"], want) and np.array_equal(p.arrays["seg_lo"], lo) and np.array_equal(p.arrays["seg_hi"], hi), name
            assert np.array_equal(p.arrays["hub_seg_ptr"], ptr) and p.scalars["n_seg"] == lo.shape[0], name
        else:
            assert all(p.arrays[k].shape[0] == 0 for k in ("hubidx", "seg_lo", "seg_hi", "hub_seg_ptr")) and p.scalars["n_seg"] == 0, name
        for i in range(3):
            if p.scalars["pers_present"][i]:
                _check_pers64(p, i, hub_t, seg, max_items, max_partials)
            else:
                assert all(p.arrays[f"{a}{16 << i}"] is None for a in ("persmap", "pershub", "perssegptr", "perssegitem")), name
                assert p.scalars["perslds"][i] == 0 and p.scalars["persitems"][i] == 0, name
        if n > max_rows:
            assert p.scalars["pers_present"] == [0, 0, 0], name
        _check_persg(p, hub_t, seg)
        p.close()


# --------------------------------------------------------------------------- the edge tables: src, rev, symmetric
def _edge_tables_hold(p, name):
    """the tables of a symmetric pattern, against the CSR itself and against tests/dmp_grad_model.py's restatement"""
    from dmp_grad_model import tables
    src, rev = p.src.astype(np.int64), p.rev.astype(np.int64)
    assert p.src.dtype == p.rev.dtype == np.int32 and src.shape == rev.shape == p.ci.shape, name
    assert np.array_equal(src, np.repeat(np.arange(p.n), np.diff(p.rp))), name
    assert p.symmetric, name
    assert np.array_equal(p.ci[rev], src) and np.array_equal(src[rev], p.ci) and np.array_equal(rev[rev], np.arange(rev.shape[0])), name
    want_src, want_rev = tables(p.rp, p.ci)
    assert np.array_equal(src, want_src) and np.array_equal(rev, want_rev), name


def _rows(*rows):
    """CSR of explicit rows of ascending columns"""
    return np.cumsum([0] + [len(r) for r in rows]).astype(np.int32), np.array([c for r in rows for c in r], np.int32)


SMALL = {"isolated_middle": _rows([1], [0], [], [4], [3]),                      # node 2 has no entry
         "path5_loop2": _rows([1], [0, 2], [1, 2, 3], [2, 4], [3]),             # a self-loop on node 2
         "rows_1_2_3": _rows([1], [0, 2], [1, 3, 4], [2], [2])}                 # both ends of the search


def test_edge_tables(lib, graphs):
    for name, (rp, ci) in {**graphs, **SMALL}.items():
        p = Plan(lib, rp, ci)
        _edge_tables_hold(p, name)
        p.close()
    p = Plan(lib, *graphs["single_node"])
    assert p.src.shape == p.rev.shape == (0,) and p.symmetric
    p.close()
    p = Plan(lib, *SMALL["path5_loop2"])
    assert p.ci[4] == 2 and p.src[4] == 2 and p.rev[4] == 4                     # the diagonal entry is its own reverse
    p.close()


def _karate_less_one(graphs):
    """(rowptr, col, u, v): karate without the directed entry (u, v), taken from the middle of a row"""
    rp, ci = graphs["karate"]
    row = int(np.argmax(np.diff(rp) >= 3))
    k = int(rp[row]) + 1                                                        # neither end of the row
    rp2 = rp.copy()
    rp2[row + 1:] -= 1
    return rp2, np.delete(ci, k), row, int(ci[k])


def test_edge_tables_of_an_asymmetric_pattern(lib, graphs):
    """karate with one directed entry taken out of the middle of a row: its opposite has no reverse, every other entry does"""
    rp2, ci2, u, v = _karate_less_one(graphs)
    p = Plan(lib, rp2, ci2)
    assert not p.error and not p.symmetric
    src, rev = p.src.astype(np.int64), p.rev.astype(np.int64)
    assert np.array_equal(src, np.repeat(np.arange(p.n), np.diff(p.rp)))
    lost = np.flatnonzero(rev == -1)
    assert lost.shape == (1,) and (src[lost[0]], p.ci[lost[0]]) == (v, u)      # the entry (v, u), whose reverse (u, v) is gone
    ok = rev >= 0
    assert np.all(rev[ok] < rev.shape[0])
    assert np.array_equal(p.ci[rev[ok]], src[ok]) and np.array_equal(src[rev[ok]], p.ci[ok]) and np.array_equal(rev[rev[ok]], np.flatnonzero(ok))
    p.close()


def _searched_rev(rp, ci):
    """rev by the binary search every handle has used (lo / hi / mid over the row of col[p], for the column src[p]), whatever
    the row's order: what the plan has to return for a CSR whose rows do not ascend, which gnode_graph_create accepts"""
    rev = np.full(len(ci), -1, np.int32)
    for u in range(len(rp) - 1):
        for p in range(rp[u], rp[u + 1]):
            lo, hi = int(rp[ci[p]]), int(rp[ci[p] + 1]) - 1
            while lo <= hi:
                mid = (lo + hi) >> 1
                if ci[mid] == u:
                    rev[p] = mid
                    break
                lo, hi = (mid + 1, hi) if ci[mid] < u else (lo, mid - 1)
    return rev


UNORDERED = {"descending_row": _rows([1, 2, 3], [0], [0], [0, 4, 2], [3]),     # row 3 does not ascend: the search misses (3, 0)
             "duplicate_column": _rows([1, 1, 2], [0, 2], [0, 1]),              # (0, 1) twice: the search settles on one of them
             "equal_neighbours_late": _rows([1], [0, 2], [1, 3, 3], [2])}


def test_edge_tables_of_rows_that_do_not_ascend(lib, graphs):
    """the search's answer, entry for entry, where the plan cannot take the one-pass merge -- and on the ordered graphs too"""
    for name, (rp, ci) in {**UNORDERED, **SMALL, "karate": graphs["karate"], "karate_less_one": _karate_less_one(graphs)[:2]}.items():
        p = Plan(lib, rp, ci)
        assert not p.error, name
        want = _searched_rev(p.rp, p.ci)
        assert np.array_equal(p.rev, want) and p.symmetric == bool((want >= 0).all()), name
        assert np.array_equal(p.src, np.repeat(np.arange(p.n), np.diff(p.rp))), name
        p.close()
    assert (_searched_rev(*UNORDERED["descending_row"]) == -1).any()


def test_plan_unit_under_sanitizers(tmp_path, graphs):
    """the plan unit and tests/graph_plan_sanitized_main.cpp, a program of its own, built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run once over every graph above: no report, and the tables' summary is the expected one"""
    small = {**SMALL, **UNORDERED, "karate_less_one": _karate_less_one(graphs)[:2]}
    cases = {**graphs, **small}
    with open(tmp_path / "graphs.txt", "w") as f:
        for rp, ci in cases.values():
            f.write(f"{len(rp) - 1} {len(ci)}\n{' '.join(map(str, rp))}\n{' '.join(map(str, ci))}\n")
    exe = str(tmp_path / "plan_sanitized")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC, "-o", exe,
                    os.path.join(CSRC, "gnode_graph_plan.cpp"), os.path.join(HERE, "graph_plan_sanitized_main.cpp")], check=True)
    run = subprocess.run([exe, str(tmp_path / "graphs.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    lost = {name: int((_searched_rev(rp, ci) < 0).sum()) if name in small else 0 for name, (rp, ci) in cases.items()}
    assert lost["karate_less_one"] == 1 and lost["descending_row"] > 0
    assert run.stdout.split("\n")[:-1] == [f"{len(cases[name][1])} {int(k == 0)} {k}" for name, k in lost.items()]


# --------------------------------------------------------------------------- argument checks, through the library
def test_graph_create_argument_checks():
    """the parent's messages, word for word; no HIP call is reached (this runs without a GPU)"""
    from gnode import _lib
    from gnode.build import build_lib
    build_lib()
    L = _lib.load()

    def create(rp, ci, nnz=None):
        rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
        out = C.c_void_p()
        st = L.gnode_graph_create(rp.ctypes.data, ci.ctypes.data, rp.shape[0] - 1, int(rp[-1]) if nnz is None else nnz, C.byref(out))
        return st, L.gnode_last_error().decode()

    assert create([0, 2, 1, 3], [1, 2, 0]) == (-1, "gnode_graph_create: rowptr not monotone at 1")
    assert create([0, 1, 2], [1, 2]) == (-1, "gnode_graph_create: col[1]=2 out of range")
    assert create([0, 1, 2], [1, -1]) == (-1, "gnode_graph_create: col[1]=-1 out of range")
    assert create([0, 1, 2], [1, 0], nnz=3) == (-1, "gnode_graph_create: rowptr[0] != 0 or rowptr[n] != nnz")
    assert create([1, 1, 2], [1, 0]) == (-1, "gnode_graph_create: rowptr[0] != 0 or rowptr[n] != nnz")
