"""GPU: outbreak sizes per candidate intervention (gnode_dmp_outbreak_sizes_f32 through gnode.dmp.outbreak_sizes, the greedy
helpers and the C entry).

The yardstick is the existing `dmp_batch`, which the tests of test_gpu_dmp_batch.py pin to the reference's vectors, on one
`InitialState` per candidate -- the base start with that node's row replaced by (0, 1, 0) (seed) or (0, 0, 1) (immunise), the
base itself for -1 -- and from its float32 marginals (out.double() * value.double()).sum(nodes).  The device computes the same
float32 marginals, and the product of two floats is exact in a double, so only the order of the n additions differs.  THE
BAR, derived and not measured: each side's fp64 summation of n terms errs by at most (n - 1) * 2^-53 * sum |term|, together less
than
    |gpu - ref| <= n * 2^-52 * sum_k |value_k * P^k_j|
(the sum of absolute values because Pi = 1 - Ps - Pr can round below 0).  Which form serves a graph is asked from
gnode_dmp_outbreak_lds_bytes, not restated here.

Measured on an MI355X (the figures this file prints): the largest |gpu - ref| / sum |term| was 4.1e-16 against bars of 1.1e-15
(n = 5) to 6.7e-13 (n = 3001); the end-to-end infections were within 6.7e-7 of the float64 model."""
import functools

import numpy as np
import pytest

import dmp_grad_model
from baseline_cases import DMP_CASES, assert_candidates_parents, candidates_entry, er as _er
from sir_cases import dev  # noqa: F401

pytestmark = pytest.mark.gpu

LDS_WORKGROUP = 160 * 1024          # what a gfx950 workgroup may declare
HORIZONS = [2, 8]                   # 2: no edge pass at all
N_BIG = 300                         # > 256: a candidate's nodes span two blocks of the general form, so the partial add runs
ONE_WORKGROUP, GENERAL = ["er34", "isolated", "nnz0"], ["hub", "big_er"]
FORM_CASE = {"one_workgroup": "er34", "general": "big_er"}
ACTIONS = {"seed": 0, "immunise": 1}
TRIPLE = {"seed": (0.0, 1.0, 0.0), "immunise": (0.0, 0.0, 1.0)}
ARG, WORKSPACE = -1, -3             # GNODE_ERR_ARG, GNODE_ERR_WORKSPACE of include/gnode.h


def _outbreak_lds_bytes(rp, ci):
    from gnode import _lib
    from gnode.graph import DeviceGraph
    g = DeviceGraph(rp, ci)
    return int(_lib.load().gnode_dmp_outbreak_lds_bytes(g.handle))


@functools.lru_cache(maxsize=None)
def big_er():
    """(rp, ci, lds bytes, lds bytes of the graph with one edge fewer): the smallest ER graph on N_BIG nodes that the
    one-workgroup form does not serve, by the library's own answer."""
    def at(m):
        rp, ci, _ = _er(N_BIG, m, 40)
        return rp, ci, _outbreak_lds_bytes(rp, ci)
    lo, hi = 3000, 6000                                             # lo fits, hi does not
    assert at(lo)[2] <= LDS_WORKGROUP < at(hi)[2]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if at(mid)[2] <= LDS_WORKGROUP else (lo, mid)
    return at(hi) + (at(lo)[2],)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(rp, ci, w, gam, seeds) of a named case, float32 tables, read-only.  er34 is dmp_grad_model's: a third of the weights
    0, gamma at 0 and at 1; no case has a weight of 1, where the forward is not finite."""
    if name == "big_er":
        rp, ci = big_er()[:2]
        s = 5.0 * N_BIG / len(ci)                                   # sized to the mean degree: neither dies out nor saturates
        c = dict(rp=rp, ci=ci, w=dmp_grad_model.weights(len(ci), 0.05 * s, 0.4 * s, 21), gam=dmp_grad_model.gammas(N_BIG, 22), seeds=[5, 250])
    else:
        c = dmp_grad_model.GRAPHS[name]() if name == "er34" else DMP_CASES[name]()
    out = dict(rp=np.asarray(c["rp"]), ci=np.asarray(c["ci"]), w=np.asarray(c["w"], np.float32), gam=np.asarray(c["gam"], np.float32))
    assert not (out["w"] == 1.0).any()
    for a in out.values():
        a.setflags(write=False)
    out["seeds"] = tuple(int(s) for s in c["seeds"])
    assert len(out["seeds"]) > 0
    return out


def _n(name):
    return len(case(name)["rp"]) - 1


def _matrix(c):
    import scipy.sparse as sp
    n = len(c["rp"]) - 1
    return sp.csr_matrix((c["w"].astype(np.float64), c["ci"], c["rp"]), shape=(n, n))


def cand_list(n):
    """non-contiguous, unsorted, with a repeat (positions 1 and 3), and -1 = "no change" last"""
    return (n - 1, 3, n // 2, 3, 0, -1)


@functools.lru_cache(maxsize=None)
def base_start(name, kind):
    """float32 [n, 3], read-only: "mixed" -- dmp_grad_model.mixed_state -- or "crisp" -- the case's seeds infected."""
    n = _n(name)
    p = dmp_grad_model.mixed_state(n, 50) if kind == "mixed" else dmp_grad_model.seed_state(n, case(name)["seeds"])
    p = np.ascontiguousarray(p, dtype=np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def values(name, seed=7):
    """float32 [n] in [0, 3), a tenth of them exactly 0, read-only"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.0, 3.0, _n(name)).astype(np.float32)
    v[rng.random(_n(name)) < 0.1] = 0.0
    v.setflags(write=False)
    return v


def starts_of(base, cands, action):
    """one InitialState per candidate: the base with that node's row replaced; an id outside the graph leaves it as it is"""
    from gnode.ode_nn import initial_state
    out = []
    for k in cands:
        p = np.array(base, dtype=np.float64)
        if 0 <= k < len(p):
            p[k] = TRIPLE[action]
        out.append(initial_state(p))
    return out


def yardstick(c, base, cands, action, value, T):
    """(ref, mag): `dmp_batch` on the candidates' starts, its float32 marginals times `value` summed over the nodes in float64,
    and the same sum of absolute values for the bar: float64 host arrays [C, T, 3]."""
    import torch
    from gnode.dmp import dmp_batch
    out = dmp_batch(_matrix(c), starts_of(base, cands, action), c["gam"], T)
    assert torch.isfinite(out).all()
    v = torch.ones(out.shape[2], dtype=torch.float32) if value is None else torch.from_numpy(np.array(value, dtype=np.float32))
    v = v.to(out.device).double().view(1, 1, -1, 1)
    return (out.double() * v).sum(2).cpu().numpy(), (out.double().abs() * v).sum(2).cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(name, T, action, kind, valued):
    """The yardstick of a named case on `cand_list`, computed once and read-only."""
    ref = yardstick(case(name), base_start(name, kind), cand_list(_n(name)), action, values(name) if valued else None, T)
    for a in ref:
        a.setflags(write=False)
    return ref


def assert_meets_the_bar(got, ref, n, what):
    got, (ref, mag) = np.asarray(got, np.float64), ref
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err, bar = np.abs(got - ref), n * 2.0 ** -52 * mag
    print(f"{what}: max |gpu - ref| / sum|term| = {np.max(err / np.maximum(mag, 1e-300)):.3e}, bar {n * 2.0 ** -52:.3e}")
    assert (err <= bar).all(), f"{what}: {np.max(err - bar):.3e} over the bar"


class Entry:
    """gnode_dmp_outbreak_sizes_f32 on one graph with device tensors of the caller's making."""

    def __init__(self, rp, ci, dev):
        from gnode import _lib
        from gnode.graph import DeviceGraph
        self.lib, self.dev, self.g = _lib.load(), dev, DeviceGraph(rp, ci)

    def need(self, C, T):
        return int(self.lib.gnode_dmp_outbreak_workspace_bytes(self.g.handle, C, T))

    def one_workgroup(self):
        return int(self.lib.gnode_dmp_outbreak_lds_bytes(self.g.handle)) <= LDS_WORKGROUP

    def up(self, a, dtype=np.float32):
        import torch
        if a is None:
            return None
        a = np.array(a, dtype=dtype, order="C")                     # (a copy: the cases' arrays are read-only)
        return None if a.size == 0 else torch.from_numpy(a).to(self.dev)       # (no edge, no table)

    def call(self, w, gam, init, cand, C, action, value, T, sizes, ws, nbytes=None):
        from gnode import _lib
        return self.lib.gnode_dmp_outbreak_sizes_f32(self.g.handle, _lib.ptr(w), _lib.ptr(gam), _lib.ptr(init), _lib.ptr(cand), C, action,
                                                     _lib.ptr(value), T, _lib.ptr(sizes), _lib.ptr(ws),
                                                     0 if ws is None else ws.numel() if nbytes is None else nbytes, _lib.stream_ptr())

    def sizes(self, c, base, cands, action, value, T, ws=None):
        """a served call on the tables of case dict `c`: the float64 device tensor [C, T, 3]"""
        import torch
        C = len(cands)
        ws = torch.empty(self.need(C, T), dtype=torch.uint8, device=self.dev) if ws is None else ws
        out = torch.full((C, T, 3), float("nan"), dtype=torch.float64, device=self.dev)
        rc = self.call(self.up(c["w"]), self.up(c["gam"]), self.up(base), self.up(cands, np.int32), C, ACTIONS[action], self.up(value), T,
                       out, ws)
        assert rc == 0, self.lib.gnode_last_error().decode()
        return out


# ------------------------------------------------------------------ which form serves which case
def test_which_form_serves_which_case(dev):
    sizes = {name: _outbreak_lds_bytes(case(name)["rp"], case(name)["ci"]) for name in ONE_WORKGROUP + GENERAL}
    for name in ONE_WORKGROUP:
        assert 0 < sizes[name] <= LDS_WORKGROUP, name
    for name in GENERAL:
        assert sizes[name] > LDS_WORKGROUP, name
    assert np.diff(case("hub")["rp"]).max() > 256                   # a long serial row
    assert np.diff(case("isolated")["rp"]).min() == 0 and len(case("nnz0")["ci"]) == 0      # empty rows, no edges
    assert N_BIG > 256 and big_er()[3] <= LDS_WORKGROUP < big_er()[2]                        # the smallest that does not fit
    from gnode import _lib
    e = Entry(case("er34")["rp"], case("er34")["ci"], dev)
    batch = int(_lib.load().gnode_dmp_batch_lds_bytes(e.g.handle))
    assert sizes["er34"] == batch + 2 * 3 * 16 * 8                  # the batch arrays | three sums of 16 waves, two steps' worth
    assert e.need(1, 8) == e.need(50, 8) == 256                     # the one-workgroup form needs no room per candidate
    e = Entry(case("big_er")["rp"], case("big_er")["ci"], dev)
    assert e.need(1, 8) < e.need(2, 8) < e.need(2, 9)
    assert e.need(0, 8) == 0 and e.need(3, 1) == 0


# ------------------------------------------------------------------ the bar, on every case, horizon, action, start and value
@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("name", ONE_WORKGROUP + GENERAL)
def test_sizes_meet_the_bar(name, T, dev):
    import torch
    c, n = case(name), _n(name)
    e = Entry(c["rp"], c["ci"], dev)
    assert e.one_workgroup() == (name in ONE_WORKGROUP)
    many = cand_list(n)
    assert many[-1] == -1 and many[1] == many[3]
    for action in ACTIONS:
        for kind in ("mixed", "crisp"):
            for valued in (False, True):
                what = f"{name} T={T} {action} {kind} start, value {'random' if valued else 'null'}"
                base, value = base_start(name, kind), values(name) if valued else None
                ref = reference(name, T, action, kind, valued)
                got = e.sizes(c, base, many, action, value, T)
                assert got.dtype == torch.float64 and got.shape == (len(many), T, 3)
                assert_meets_the_bar(got.cpu().numpy(), ref, n, what)            # (row -1 against dmp_batch on the base start)
                assert torch.equal(got[1], got[3])                  # the repeated id gives identical rows
                one = e.sizes(c, base, many[:1], action, value, T)  # C = 1: the bits of the same candidate in the larger call
                assert torch.equal(one[0], got[0]), what
                nothing = e.sizes(c, base, [-1, n, 2 ** 31 - 1, -2 ** 31], action, value, T)     # an id outside the graph matches no node
                assert all(torch.equal(nothing[i], got[-1]) for i in range(4)), what


# ------------------------------------------------------------------ exact results
@pytest.mark.parametrize("name", ["er34", "nnz0", "big_er"])
def test_row_0_of_a_crisp_start_is_the_integer_triple(name, dev):
    c, n, T = case(name), _n(name), 8
    seeds = set(c["seeds"])
    e = Entry(c["rp"], c["ci"], dev)
    many = cand_list(n)
    for action in ACTIONS:
        got = e.sizes(c, base_start(name, "crisp"), many, action, None, T).cpu().numpy()
        for i, k in enumerate(many):
            infected = seeds | {k} if action == "seed" and k >= 0 else seeds - {k} if action == "immunise" else seeds
            removed = 1 if action == "immunise" and k >= 0 else 0
            assert got[i, 0].tolist() == [float(n - len(infected) - removed), float(len(infected)), float(removed)], (action, k)
            if name == "nnz0":                                      # no edge: nobody is ever infected by anybody
                assert (got[i, :, 0] == float(n - len(infected) - removed)).all(), (action, k)


def _path(n, w):
    rp = np.concatenate([[0], np.cumsum([1] + [2] * (n - 2) + [1])]).astype(np.int32)
    ci = np.asarray([j for i in range(n) for j in (i - 1, i + 1) if 0 <= j < n], dtype=np.int32)
    return dict(rp=rp, ci=ci, w=np.full(len(ci), w, np.float32))


def test_an_immunised_node_cuts_a_path(dev):
    """A path of 9 nodes with the seed at node 0: with node 1 immunised nothing beyond it is ever reached, so the S sum is
    exactly 7 at every t (the messages out of a node that never holds infection stay exactly 1)."""
    n, T = 9, 8
    c = dict(_path(n, 0.5), gam=np.full(n, 0.3, np.float32))
    e = Entry(c["rp"], c["ci"], dev)
    got = e.sizes(c, dmp_grad_model.seed_state(n, [0]), [1, 4, -1], "immunise", None, T).cpu().numpy()
    assert got[0, :, 0].tolist() == [7.0] * T
    assert got[0, :, 2].min() >= 1.0                                # the immunised node itself
    assert got[1, 0, 0] == 7.0 and got[1, T - 1, 0] < 7.0           # node 4 immunised: 1, 2, 3 are reached
    assert got[2, 0, 0] == 8.0 and got[2, T - 1, 0] < 8.0           # nothing immunised
    assert got[2, T - 1, 1] + got[2, T - 1, 2] > got[1, T - 1, 1] + got[1, T - 1, 2] - 1.0 > got[0, T - 1, 1] + got[0, T - 1, 2] - 1.0


# ------------------------------------------------------------------ independence, reproducibility, state
@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_a_candidates_rows_do_not_depend_on_their_company(form, dev):
    import torch
    from gnode.dmp import DmpGraph, outbreak_sizes
    from gnode.ode_nn import initial_state
    name = FORM_CASE[form]
    c, n, T = case(name), _n(name), 8
    base, value = base_start(name, "mixed"), values(name)
    many = list(cand_list(n))
    e = Entry(c["rp"], c["ci"], dev)
    full = e.sizes(c, base, many, "immunise", value, T)
    for i, k in enumerate(many):
        assert torch.equal(e.sizes(c, base, [k], "immunise", value, T)[0], full[i]), f"candidate {k} alone"
    G, start = DmpGraph(_matrix(c)), initial_state(base)
    budget = e.need(2, T)                                           # two candidates per chunk where the workspace grows with C
    assert (e.need(len(many), T) > budget) == (form == "general")
    kw = dict(candidates=many, action="immunise", start=start, value=value)
    assert torch.equal(outbreak_sizes(G, c["gam"], T, budget_bytes=budget, **kw), full)
    assert torch.equal(outbreak_sizes(G, c["gam"], T, **kw), full)                           # one chunk
    with pytest.raises(ValueError):
        outbreak_sizes(G, c["gam"], T, budget_bytes=e.need(1, T) - 1, **kw)
    every = outbreak_sizes(G, c["gam"], T, action="immunise", start=start, value=value)     # the default: every node
    assert every.shape == (n, T, 3) and every.device.type == dev.type
    assert all(torch.equal(every[k], full[i]) for i, k in enumerate(many[:-1]))


@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_reproducible_and_no_state_is_carried_over_in_the_workspace(form, dev):
    import torch
    name = FORM_CASE[form]
    c, n, T = case(name), _n(name), 8
    base, value = base_start(name, "mixed"), values(name)
    many = list(cand_list(n))
    e = Entry(c["rp"], c["ci"], dev)
    first = e.sizes(c, base, many[:2], "seed", value, T)
    assert torch.equal(e.sizes(c, base, many[:2], "seed", value, T), first)      # the same call twice
    ws = torch.full((e.need(len(many), 9),), 0xFF, dtype=torch.uint8, device=dev)      # NaNs, should anything read before it writes
    other = dict(c, gam=(c["gam"] * np.float32(0.5)).astype(np.float32))
    larger = e.sizes(other, base_start(name, "crisp"), many, "immunise", values(name, 8), 9, ws=ws)      # a larger call, other numbers
    assert torch.isfinite(larger).all()
    assert torch.equal(e.sizes(c, base, many[:2], "seed", value, T, ws=ws), first)           # ... then the first one on its workspace


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_refusals_leave_sizes_untouched_and_a_good_call_is_served(form, dev):
    import torch
    name = FORM_CASE[form]
    c, n, T = case(name), _n(name), 8
    rp, ci = c["rp"], c["ci"]
    nnz = len(ci)
    many = cand_list(n)
    C = len(many)
    e = Entry(rp, ci, dev)
    w, gam, init, cand, value = e.up(c["w"]), e.up(c["gam"]), e.up(base_start(name, "mixed")), e.up(many, np.int32), e.up(values(name))
    need = e.need(C, T)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    sizes = torch.full((C, T, 3), float("nan"), dtype=torch.float64, device=dev)
    assert e.call(w, gam, init, cand, C, 0, value, T, sizes, ws, need - 1) == WORKSPACE
    assert e.call(w, gam, init, cand, 0, 0, value, T, sizes, ws) == ARG
    assert e.call(w, gam, init, cand, -3, 0, value, T, sizes, ws) == ARG
    assert e.call(w, gam, init, cand, C, 0, value, 1, sizes, ws) == ARG
    for action in (2, -1):
        assert e.call(w, gam, init, cand, C, action, value, T, sizes, ws) == ARG, action
    for missing in ("w", "gam", "init", "cand", "sizes", "ws"):
        a = dict(w=w, gam=gam, init=init, cand=cand, sizes=sizes, ws=ws)
        a[missing] = None
        assert e.call(a["w"], a["gam"], a["init"], a["cand"], C, 0, value, T, a["sizes"], a["ws"], need) == ARG, missing
    if form == "general":                                           # too many candidates for the grid: refused before anything is read
        assert e.call(w, gam, init, cand, 2 ** 31 - 1, 0, value, T, sizes, ws) == ARG
        assert "too many" in e.lib.gnode_last_error().decode()
    k = nnz // 2                                                    # one directed entry out of the middle of the CSR
    row = int(np.searchsorted(rp, k, side="right") - 1)
    rp2 = rp.copy(); rp2[row + 1:] -= 1
    e2 = Entry(rp2, np.delete(ci, k), dev)
    ws2 = torch.empty(e2.need(C, T), dtype=torch.uint8, device=dev)
    assert e2.call(e.up(np.delete(c["w"], k)), gam, init, cand, C, 0, value, T, sizes, ws2) == ARG
    assert "symmetric" in e2.lib.gnode_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(sizes).all())
    assert e.call(w, gam, init, cand, C, 0, value, T, sizes, ws) == 0, e.lib.gnode_last_error().decode()   # value present ...
    assert_meets_the_bar(sizes.cpu().numpy(), reference(name, T, "seed", "mixed", True), n, f"{name} after the refusals")
    assert e.call(w, gam, init, cand, C, 0, None, T, sizes, ws) == 0, e.lib.gnode_last_error().decode()    # ... and null: served
    assert_meets_the_bar(sizes.cpu().numpy(), reference(name, T, "seed", "mixed", False), n, f"{name} after the refusals, value null")


# ------------------------------------------------------------------ end to end
def model_infections(c, base, action, cands, T):
    """The float64 model's `infections` per candidate: dmp_grad_model.forward from the base with the candidate's row replaced."""
    import torch
    n = len(c["rp"]) - 1
    src, rev = (torch.from_numpy(a) for a in dmp_grad_model.tables(c["rp"], c["ci"]))
    f64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))   # noqa: E731
    got = []
    for k in cands:
        p = np.array(base, dtype=np.float64)
        if k >= 0:
            p[k] = TRIPLE[action]
        out = dmp_grad_model.forward(src, rev, n, f64(c["w"]), f64(c["gam"]), f64(p), T).sum(1)
        got.append(float(out[-1, 1] + out[-1, 2] - out[0, 2]))
    return np.asarray(got)


def _from_edges(n, edges, w, gamma):
    import scipy.sparse as sp
    u, v = np.asarray(edges).T
    A = sp.coo_matrix((np.ones(2 * len(edges)), (np.r_[u, v], np.r_[v, u])), shape=(n, n)).tocsr()
    A.sort_indices()
    return dict(rp=A.indptr.astype(np.int32), ci=A.indices.astype(np.int32), w=np.full(A.nnz, w, np.float32), gam=np.full(n, gamma, np.float32))


def barbell():
    """cliques {0..4} and {6..10} joined through node 5, which is joined to 4 and to 6; all weights 0.4, gamma 0.3"""
    clique = lambda ids: [(a, b) for a in ids for b in ids if a < b]         # noqa: E731
    return _from_edges(11, clique(range(5)) + clique(range(6, 11)) + [(4, 5), (5, 6)], 0.4, 0.3)


def star_and_path():
    """hub 0 with leaves 1..6, and the path 6-7-8-9-10-11 off leaf 6; all weights 0.3, gamma 0.2"""
    return _from_edges(12, [(0, k) for k in range(1, 7)] + [(k, k + 1) for k in range(6, 11)], 0.3, 0.2)


def test_greedy_immunisation_cuts_the_barbell_at_the_clique(dev):
    """Seed at node 0, maxTime 12.  The float64 model: immunising node 4 leaves 3.853 infections, node 5 4.953, doing nothing
    10.504; a second round then picks one of the symmetric nodes 1, 2, 3."""
    from gnode.dmp import DmpGraph, greedy_immunisation, infections, outbreak_sizes
    c, n, T = barbell(), 11, 12
    base = dmp_grad_model.seed_state(n, [0])
    pool = list(range(1, n))
    model = model_infections(c, base, "immunise", pool + [-1], T)
    order = np.argsort(model, kind="stable")
    print(f"model: immunise {pool[order[0]]}: {model[order[0]]:.3f}, then {pool[order[1]]}: {model[order[1]]:.3f}; nothing: {model[-1]:.3f}")
    assert pool[order[0]] == 4 and abs(model[order[0]] - 3.853) < 1e-3 and abs(model[pool.index(5)] - 4.953) < 1e-3
    assert abs(model[-1] - 10.504) < 1e-3 and model[order[1]] - model[order[0]] > 0.05
    G = DmpGraph(_matrix(c))
    got = infections(outbreak_sizes(G, c["gam"], T, candidates=pool + [-1], action="immunise", start=[0])).cpu().numpy()
    print(f"gpu - model: max {np.abs(got - model).max():.3e}")
    assert np.abs(got - model).max() < 1e-3
    picked = greedy_immunisation(G, [0], c["gam"], T, 1)
    assert [k for k, _ in picked] == [4] and picked[0][1] == got[pool.index(4)]
    base2 = np.array(base); base2[4] = TRIPLE["immunise"]
    pool2 = [k for k in pool if k != 4]
    model2 = model_infections(c, base2, "immunise", pool2, T)
    best2 = np.sort(model2)
    print(f"model, round 2: {dict(zip(pool2, np.round(model2, 3)))}")
    assert {pool2[i] for i in np.flatnonzero(model2 - best2[0] < 1e-9)} == {1, 2, 3} and best2[3] - best2[0] > 0.05
    two = greedy_immunisation(G, [0], c["gam"], T, 2)
    assert two[0] == picked[0] and two[1][0] in (1, 2, 3) and abs(two[1][1] - best2[0]) < 1e-3
    assert two[1][1] < two[0][1]


def test_greedy_seeds_takes_the_hub_then_the_far_path(dev):
    """maxTime 6.  The float64 model: round 1 node 0 with 5.356 infections against 4.473 for the runner-up; round 2 node 9 with
    8.143 against 8.013."""
    from gnode.dmp import DmpGraph, greedy_seeds
    c, n, T = star_and_path(), 12, 6
    base = dmp_grad_model.seed_state(n, [])
    pool = list(range(n))
    model = model_infections(c, base, "seed", pool, T)
    order = np.argsort(-model, kind="stable")
    print(f"model, round 1: {pool[order[0]]}: {model[order[0]]:.3f} against {pool[order[1]]}: {model[order[1]]:.3f}")
    assert pool[order[0]] == 0 and abs(model[order[0]] - 5.356) < 1e-3 and abs(model[order[1]] - 4.473) < 1e-3
    assert model[order[0]] - model[order[1]] > 0.05
    base2 = np.array(base); base2[0] = TRIPLE["seed"]
    pool2 = pool[1:]
    model2 = model_infections(c, base2, "seed", pool2, T)
    order2 = np.argsort(-model2, kind="stable")
    print(f"model, round 2: {pool2[order2[0]]}: {model2[order2[0]]:.3f} against {pool2[order2[1]]}: {model2[order2[1]]:.3f}")
    assert pool2[order2[0]] == 9 and abs(model2[order2[0]] - 8.143) < 1e-3 and abs(model2[order2[1]] - 8.013) < 1e-3
    assert model2[order2[0]] - model2[order2[1]] > 0.05
    got = greedy_seeds(DmpGraph(_matrix(c)), c["gam"], T, 2)
    assert [k for k, _ in got] == [0, 9], got
    assert abs(got[0][1] - model[0]) < 1e-3 and abs(got[1][1] - model2[pool2.index(9)]) < 1e-3


# ------------------------------------------------------------------ the parent's bits
PARENT_CASES = [(name, T) for name in ONE_WORKGROUP + GENERAL for T in HORIZONS]


def parent_entries(name, T, dev):
    """[(key, entry)] of tests/golden/dmp_candidates_parent.json for one case and horizon: both actions on the mixed start, with
    and without `value`, on `cand_list`'s candidates (the last of them -1)."""
    c, n = case(name), _n(name)
    e = Entry(c["rp"], c["ci"], dev)
    many = cand_list(n)
    sizes = dict(workspace_bytes=e.need(len(many), T), lds_bytes=e.lib.gnode_dmp_outbreak_lds_bytes(e.g.handle))
    return [(f"outbreak/{name}/T{T}/{action}/{'valued' if valued else 'null'}",
             candidates_entry(e.sizes(c, base_start(name, "mixed"), many, action, values(name) if valued else None, T), **sizes))
            for action in ACTIONS for valued in (False, True)]


@pytest.mark.parametrize("name,T", PARENT_CASES)
def test_sizes_are_the_parents_bits(name, T, dev):
    """tests/golden/dmp_candidates_parent.json: what the library of commit 40c1952 returned on an MI355X, when this entry had
    kernels and a host side of its own.  Equality of digests, of the workspace and of the LDS the library asks for."""
    assert_candidates_parents(parent_entries(name, T, dev))
