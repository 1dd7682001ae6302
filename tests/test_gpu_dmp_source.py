"""GPU: source inference from one snapshot (gnode_dmp_source_scores_f32 through gnode.dmp.source_scores and through the C entry).

The yardstick is the existing `dmp_batch` on the same candidates' one-hot starts, which the tests of test_gpu_dmp_batch.py pin to
the reference's vectors: from its float32 marginals torch.log(out.clamp(floor, 1).double()), gathered by `obs` and summed over
the observed nodes.  The device computes the same float32 marginals, so only the rounding of the logarithm and the order of
the sum differ.  THE BAR, derived and not measured: each of the two logarithms is within one unit in the last place of the
true one, 2^-52 relative at the most, so two terms differ by at most 2 * 2^-52 of their size; every term is <= 0, so nothing
cancels and the same holds for the sums; each of the two fp64 summations of n_obs terms of one sign adds at most
(n_obs - 1) * 2^-53 of the sum.  Together less than
    |gpu - ref| <= (n_obs + 4) * 2^-52 * |ref|.
Which form serves a graph is asked from gnode_dmp_source_lds_bytes, not restated here."""
import functools
import math

import numpy as np
import pytest

import dmp_grad_model
from baseline_cases import DMP_CASES, assert_candidates_parents, candidates_entry, er as _er
from sir_cases import dev  # noqa: F401

pytestmark = pytest.mark.gpu

LDS_WORKGROUP = 160 * 1024          # what a gfx950 workgroup may declare
FLOOR = 1e-30
HORIZONS = [2, 8]                   # 2: no edge pass at all
N_BIG = 300                         # > 256: a candidate's nodes span two blocks of the general form, so the partial add runs
ONE_WORKGROUP, GENERAL = ["er34", "isolated", "nnz0"], ["hub", "big_er"]
FORM_CASE = {"one_workgroup": "er34", "general": "big_er"}
ARG, WORKSPACE = -1, -3             # GNODE_ERR_ARG, GNODE_ERR_WORKSPACE of include/gnode.h


def _source_lds_bytes(rp, ci):
    from gnode import _lib
    from gnode.graph import DeviceGraph
    g = DeviceGraph(rp, ci)
    return int(_lib.load().gnode_dmp_source_lds_bytes(g.handle))


@functools.lru_cache(maxsize=None)
def big_er():
    """(rp, ci, lds bytes, lds bytes of the graph with one edge fewer): the smallest ER graph on N_BIG nodes that the
    one-workgroup form does not serve, by the library's own answer."""
    def at(m):
        rp, ci, _ = _er(N_BIG, m, 40)
        return rp, ci, _source_lds_bytes(rp, ci)
    lo, hi = 3000, 6000                                             # lo fits, hi does not
    assert at(lo)[2] <= LDS_WORKGROUP < at(hi)[2]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if at(mid)[2] <= LDS_WORKGROUP else (lo, mid)
    return at(hi) + (at(lo)[2],)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(rp, ci, w, gam) of a named case, float32 tables, read-only.  er34 is dmp_grad_model's: a third of the weights 0,
    gamma at 0 and at 1; no case has a weight of 1, where the forward is not finite."""
    if name == "big_er":
        rp, ci = big_er()[:2]
        s = 5.0 * N_BIG / len(ci)                                   # sized to the mean degree: neither dies out nor saturates
        c = dict(rp=rp, ci=ci, w=dmp_grad_model.weights(len(ci), 0.05 * s, 0.4 * s, 21), gam=dmp_grad_model.gammas(N_BIG, 22))
    else:
        c = dmp_grad_model.GRAPHS[name]() if name == "er34" else DMP_CASES[name]()
    out = dict(rp=np.asarray(c["rp"]), ci=np.asarray(c["ci"]), w=np.asarray(c["w"], np.float32), gam=np.asarray(c["gam"], np.float32))
    assert not (out["w"] == 1.0).any()
    for a in out.values():
        a.setflags(write=False)
    return out


def _n(name):
    return len(case(name)["rp"]) - 1


def _matrix(c):
    import scipy.sparse as sp
    n = len(c["rp"]) - 1
    return sp.csr_matrix((c["w"].astype(np.float64), c["ci"], c["rp"]), shape=(n, n))


def mixed_obs(n, seed=5):
    return np.random.default_rng(seed).choice(np.asarray([-1, 0, 1, 2], dtype=np.int32), size=n, p=[0.25, 0.35, 0.25, 0.15])


def cand_list(n):
    """non-contiguous, unsorted, with a repeat (positions 1 and 3)"""
    return (n - 1, 3, n // 2, 3, 0)


def yardstick(c, cands, obs, T, floor=FLOOR):
    """`dmp_batch` on the candidates' one-hot starts, the clamped float64 logarithm of its marginals gathered by `obs` and
    summed over the observed nodes: a float64 host array [C, T]."""
    import torch
    from gnode.dmp import dmp_batch
    out = dmp_batch(_matrix(c), [[int(k)] for k in cands], c["gam"], T)
    assert torch.isfinite(out).all()
    obs = torch.from_numpy(np.asarray(obs, dtype=np.int64)).to(out.device)
    logp = torch.log(out.clamp(float(np.float32(floor)), 1.0).double())
    seen = torch.nonzero(obs >= 0).flatten()
    idx = obs[seen].view(1, 1, -1, 1).expand(len(cands), T, -1, 1)
    return logp[:, :, seen, :].gather(3, idx)[..., 0].sum(2).cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(name, T, cands):
    """The yardstick of a named case with `mixed_obs`, computed once and read-only."""
    ref = yardstick(case(name), cands, mixed_obs(_n(name)), T)
    ref.setflags(write=False)
    return ref


def assert_meets_the_bar(got, ref, n_obs, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err, bar = np.abs(got - ref), (n_obs + 4) * 2.0 ** -52 * np.abs(ref)
    print(f"{what}: max |gpu - ref| / |ref| = {np.max(err / np.maximum(np.abs(ref), 1e-300)):.3e}, bar {(n_obs + 4) * 2.0 ** -52:.3e}")
    assert (err <= bar).all(), f"{what}: {np.max(err - bar):.3e} over the bar"


class Entry:
    """gnode_dmp_source_scores_f32 on one graph with device tensors of the caller's making."""

    def __init__(self, rp, ci, dev):
        from gnode import _lib
        from gnode.graph import DeviceGraph
        self.lib, self.dev, self.g = _lib.load(), dev, DeviceGraph(rp, ci)

    def need(self, C, T):
        return int(self.lib.gnode_dmp_source_workspace_bytes(self.g.handle, C, T))

    def one_workgroup(self):
        return int(self.lib.gnode_dmp_source_lds_bytes(self.g.handle)) <= LDS_WORKGROUP

    def up(self, a, dtype=np.float32):
        import torch
        a = np.array(a, dtype=dtype, order="C")                     # (a copy: the cases' arrays are read-only)
        return None if a.size == 0 else torch.from_numpy(a).to(self.dev)       # (no edge, no table)

    def call(self, w, gam, cand, C, obs, floor, T, scores, ws, nbytes=None):
        from gnode import _lib
        return self.lib.gnode_dmp_source_scores_f32(self.g.handle, _lib.ptr(w), _lib.ptr(gam), _lib.ptr(cand), C, _lib.ptr(obs), floor, T,
                                                    _lib.ptr(scores), _lib.ptr(ws), 0 if ws is None else ws.numel() if nbytes is None else nbytes,
                                                    _lib.stream_ptr())

    def scores(self, c, cands, obs, T, floor=FLOOR, ws=None):
        """a served call on the tables of case dict `c`: the float64 device tensor [C, T]"""
        import torch
        C = len(cands)
        ws = torch.empty(self.need(C, T), dtype=torch.uint8, device=self.dev) if ws is None else ws
        out = torch.full((C, T), float("nan"), dtype=torch.float64, device=self.dev)
        rc = self.call(self.up(c["w"]), self.up(c["gam"]), self.up(cands, np.int32), C, self.up(obs, np.int32), floor, T, out, ws)
        assert rc == 0, self.lib.gnode_last_error().decode()
        return out


# ------------------------------------------------------------------ which form serves which case
def test_which_form_serves_which_case(dev):
    sizes = {name: _source_lds_bytes(case(name)["rp"], case(name)["ci"]) for name in ONE_WORKGROUP + GENERAL}
    for name in ONE_WORKGROUP:
        assert 0 < sizes[name] <= LDS_WORKGROUP, name
    for name in GENERAL:
        assert sizes[name] > LDS_WORKGROUP, name
    assert np.diff(case("hub")["rp"]).max() > 256                   # a long serial row
    assert np.diff(case("isolated")["rp"]).min() == 0 and len(case("nnz0")["ci"]) == 0      # empty rows, no edges
    assert N_BIG > 256 and big_er()[3] <= LDS_WORKGROUP < big_er()[2]                        # the smallest that does not fit
    e = Entry(case("er34")["rp"], case("er34")["ci"], dev)
    assert e.need(1, 8) == e.need(50, 8) > 0                        # the one-workgroup form needs no room per candidate
    e = Entry(case("big_er")["rp"], case("big_er")["ci"], dev)
    assert e.need(1, 8) < e.need(2, 8) < e.need(2, 9)
    assert e.need(0, 8) == 0 and e.need(3, 1) == 0


# ------------------------------------------------------------------ the bar, on every case, horizon and candidate list
@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("name", ONE_WORKGROUP + GENERAL)
def test_scores_meet_the_bar(name, T, dev):
    import torch
    c, n = case(name), _n(name)
    obs = mixed_obs(n)
    n_obs = int((obs >= 0).sum())
    assert n_obs > 0 and set(np.unique(obs)) <= {-1, 0, 1, 2}
    e = Entry(c["rp"], c["ci"], dev)
    assert e.one_workgroup() == (name in ONE_WORKGROUP)
    many = cand_list(n)
    got = e.scores(c, many, obs, T)
    assert got.dtype == torch.float64 and got.shape == (len(many), T)
    assert_meets_the_bar(got.cpu().numpy(), reference(name, T, many), n_obs, f"{name} T={T} C={len(many)}")
    assert torch.equal(got[1], got[3])                              # the repeated id gives identical rows
    assert float(got.max()) < 0.0                                   # something is observed, and not with certainty
    one = e.scores(c, many[:1], obs, T)                             # C = 1
    assert_meets_the_bar(one.cpu().numpy(), reference(name, T, many)[:1], n_obs, f"{name} T={T} C=1")
    assert torch.equal(one[0], got[0])


@pytest.mark.parametrize("name", ["isolated", "big_er"])
def test_python_surface_meets_the_bar_with_default_candidates(name, dev):
    import torch
    from gnode.dmp import DmpGraph, source_candidates, source_scores
    c, n, T = case(name), _n(name), 8
    obs = mixed_obs(n)
    hidden = source_candidates(obs)[6:]                             # all but six of the nodes observed I or R become unobserved
    obs = np.where(np.isin(np.arange(n), hidden), -1, obs)
    cands = source_candidates(obs)
    assert len(cands) == 6 and all(obs[k] >= 1 for k in cands)
    got = source_scores(DmpGraph(_matrix(c)), obs, c["gam"], T)
    assert got.shape == (6, T) and got.dtype == torch.float64 and got.device.type == dev.type
    assert torch.equal(got, Entry(c["rp"], c["ci"], dev).scores(c, cands, obs, T))
    assert_meets_the_bar(got.cpu().numpy(), yardstick(c, cands, obs, T), int((obs >= 0).sum()), f"source_scores {name}")


# ------------------------------------------------------------------ observations
@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_nothing_observed_scores_exactly_zero(form, dev):
    import torch
    name = FORM_CASE[form]
    c, n = case(name), _n(name)
    e = Entry(c["rp"], c["ci"], dev)
    for obs in (np.full(n, -1), np.resize([-1, 3, 7, -2, 2 ** 31 - 1, -2 ** 31], n)):       # anything but 0 / 1 / 2 is "not observed"
        for T in HORIZONS:
            got = e.scores(c, cand_list(n), obs, T)
            assert bool((got == 0.0).all()) and not bool(torch.signbit(got).any())


def _path(n, w):
    rp = np.concatenate([[0], np.cumsum([1] + [2] * (n - 2) + [1])]).astype(np.int32)
    ci = np.asarray([j for i in range(n) for j in (i - 1, i + 1) if 0 <= j < n], dtype=np.int32)
    return dict(rp=rp, ci=ci, w=np.full(len(ci), w, np.float32))


@pytest.mark.parametrize("floor", [1e-30, 1e-6, 1.0])
def test_a_node_out_of_reach_contributes_log_floor(floor, dev):
    """maxTime = 3 on a path: a node observed infected at distance > 2 from the candidate has Pi exactly 0 at t <= 2, so with
    nothing else observed the score IS log((double)float32(floor))."""
    n, T = 9, 3
    c = dict(_path(n, 0.5), gam=np.full(n, 0.3, np.float32))
    obs = np.full(n, -1)
    obs[7] = 1
    e = Entry(c["rp"], c["ci"], dev)
    got = e.scores(c, [0, 4, 8, 7], obs, T, floor=floor).cpu().numpy()
    want = math.log(float(np.float32(floor)))
    for row in (0, 1):                                              # candidates 0 and 4: at distance 7 and 3
        assert got[row].tolist() == [want] * T, (row, got[row], want)
    assert got[2, 0] == want and (got[2, 1] > want or floor == 1.0)     # candidate 8, a neighbour: reached at t = 1
    assert got[3, 0] == 0.0                                         # the observed node itself as the source: Pi_0 = 1


# ------------------------------------------------------------------ independence, reproducibility, state
@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_a_candidates_row_does_not_depend_on_its_company(form, dev):
    import torch
    from gnode.dmp import DmpGraph, source_scores
    name = FORM_CASE[form]
    c, n, T = case(name), _n(name), 8
    obs = mixed_obs(n)
    many = list(cand_list(n))
    e = Entry(c["rp"], c["ci"], dev)
    chunk5 = e.scores(c, many, obs, T)
    for i, k in enumerate(many):
        assert torch.equal(e.scores(c, [k], obs, T)[0], chunk5[i]), f"candidate {k} alone"
    G = DmpGraph(_matrix(c))
    budget = e.need(2, T)                                           # two candidates per chunk where the workspace grows with C
    assert (e.need(len(many), T) > budget) == (form == "general")
    assert torch.equal(source_scores(G, obs, c["gam"], T, candidates=many, budget_bytes=budget), chunk5)
    assert torch.equal(source_scores(G, obs, c["gam"], T, candidates=many), chunk5)         # one chunk
    with pytest.raises(ValueError):
        source_scores(G, obs, c["gam"], T, candidates=many, budget_bytes=e.need(1, T) - 1)


@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_reproducible_and_no_state_is_carried_over_in_the_workspace(form, dev):
    import torch
    name = FORM_CASE[form]
    c, n, T = case(name), _n(name), 8
    obs = mixed_obs(n)
    many = list(cand_list(n))
    e = Entry(c["rp"], c["ci"], dev)
    first = e.scores(c, many[:2], obs, T)
    assert torch.equal(e.scores(c, many[:2], obs, T), first)        # the same call twice
    ws = torch.full((e.need(len(many), 9),), 0xFF, dtype=torch.uint8, device=dev)      # NaNs, should anything read before it writes
    other = dict(c, gam=(c["gam"] * np.float32(0.5)).astype(np.float32))
    larger = e.scores(other, many, mixed_obs(n, 6), 9, ws=ws)       # a larger call, other numbers
    assert torch.isfinite(larger).all()
    assert torch.equal(e.scores(c, many[:2], obs, T, ws=ws), first)     # ... then the first one on its workspace


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_refusals_leave_scores_untouched_and_a_good_call_is_served(form, dev):
    import torch
    name = FORM_CASE[form]
    c, n, T = case(name), _n(name), 4
    rp, ci = c["rp"], c["ci"]
    nnz = len(ci)
    obs_h = mixed_obs(n)
    many = cand_list(n)
    C = len(many)
    e = Entry(rp, ci, dev)
    w, gam, cand, obs = e.up(c["w"]), e.up(c["gam"]), e.up(many, np.int32), e.up(obs_h, np.int32)
    need = e.need(C, T)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    scores = torch.full((C, T), float("nan"), dtype=torch.float64, device=dev)
    assert e.call(w, gam, cand, C, obs, FLOOR, T, scores, ws, need - 1) == WORKSPACE
    assert e.call(w, gam, cand, 0, obs, FLOOR, T, scores, ws) == ARG
    assert e.call(w, gam, cand, -3, obs, FLOOR, T, scores, ws) == ARG
    assert e.call(w, gam, cand, C, obs, FLOOR, 1, scores, ws) == ARG
    for floor in (0.0, -1e-30, 1.5, float("nan"), float("inf")):
        assert e.call(w, gam, cand, C, obs, floor, T, scores, ws) == ARG, floor
    for missing in ("w", "gam", "cand", "obs", "scores", "ws"):
        a = dict(w=w, gam=gam, cand=cand, obs=obs, scores=scores, ws=ws)
        a[missing] = None
        assert e.call(a["w"], a["gam"], a["cand"], C, a["obs"], FLOOR, T, a["scores"], a["ws"], need) == ARG, missing
    if form == "general":                                           # too many candidates for the grid: refused before anything is read
        assert e.call(w, gam, cand, 2 ** 31 - 1, obs, FLOOR, T, scores, ws) == ARG
        assert "too many" in e.lib.gnode_last_error().decode()
    k = nnz // 2                                                    # one directed entry out of the middle of the CSR
    row = int(np.searchsorted(rp, k, side="right") - 1)
    rp2 = rp.copy(); rp2[row + 1:] -= 1
    e2 = Entry(rp2, np.delete(ci, k), dev)
    ws2 = torch.empty(e2.need(C, T), dtype=torch.uint8, device=dev)
    assert e2.call(e.up(np.delete(c["w"], k)), gam, cand, C, obs, FLOOR, T, scores, ws2) == ARG
    assert "symmetric" in e2.lib.gnode_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(scores).all())
    assert e.call(w, gam, cand, C, obs, FLOOR, T, scores, ws) == 0, e.lib.gnode_last_error().decode()
    assert_meets_the_bar(scores.cpu().numpy(), reference(name, T, many), int((obs_h >= 0).sum()), f"{name} after the refusals")


# ------------------------------------------------------------------ end to end
def test_the_source_of_a_path_outbreak_is_found(dev):
    """A path of 9 nodes, all weights 0.5, gamma 0.3; nodes 3 and 5 observed infected, node 4 recovered, the rest susceptible,
    maxTime 8.  The float64 model (dmp_grad_model.forward per candidate, the same clamp) puts the maximum at candidate 4, t = 2,
    2.87 ahead of the runner-up."""
    import torch
    from gnode.dmp import rank_sources, source_scores
    n, T = 9, 8
    c = dict(_path(n, 0.5), gam=np.full(n, 0.3, np.float32))
    obs = np.zeros(n, dtype=np.int64)
    obs[[3, 5]], obs[4] = 1, 2
    src, rev = (torch.from_numpy(a) for a in dmp_grad_model.tables(c["rp"], c["ci"]))
    f64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))   # noqa: E731
    model = np.empty((n, T))
    for k in range(n):
        out = dmp_grad_model.forward(src, rev, n, f64(c["w"]), f64(c["gam"]), f64(dmp_grad_model.seed_state(n, [k])), T)
        logp = torch.log(out.clamp(float(np.float32(FLOOR)), 1.0))
        model[k] = logp.gather(2, torch.from_numpy(obs).view(1, n, 1).expand(T, n, 1))[..., 0].sum(1).numpy()
    best = model.max(1)
    order = np.argsort(-best)
    print(f"model: best candidate {order[0]} at t = {model[order[0]].argmax()}, {best[order[0]] - best[order[1]]:.3f} ahead of candidate {order[1]}")
    assert order[0] == 4 and model[4].argmax() == 2
    assert best[4] - best[order[1]] > 1.0
    for cands in (None, np.arange(n)):                              # the default: the nodes observed I or R, here 3, 4, 5
        scores = source_scores(_matrix(c), obs, 0.3, T, candidates=cands)
        ids = [3, 4, 5] if cands is None else list(cands)
        assert scores.shape == (len(ids), T)
        ranked = rank_sources(scores, ids)
        assert ranked[0][:2] == (4, 2), ranked
        assert [r[0] for r in ranked] == [ids[i] for i in np.argsort(-scores.max(1).values.cpu().numpy(), kind="stable")]


# ------------------------------------------------------------------ the parent's bits
PARENT_CASES = [(name, T) for name in ONE_WORKGROUP + GENERAL for T in HORIZONS]


def parent_entries(name, T, dev):
    """[(key, entry)] of tests/golden/dmp_candidates_parent.json for one case and horizon: `cand_list`'s candidates on `mixed_obs`."""
    c, n = case(name), _n(name)
    e = Entry(c["rp"], c["ci"], dev)
    many = cand_list(n)
    sizes = dict(workspace_bytes=e.need(len(many), T), lds_bytes=e.lib.gnode_dmp_source_lds_bytes(e.g.handle))
    return [(f"source/{name}/T{T}", candidates_entry(e.scores(c, many, mixed_obs(n), T), **sizes))]


@pytest.mark.parametrize("name,T", PARENT_CASES)
def test_scores_are_the_parents_bits(name, T, dev):
    """tests/golden/dmp_candidates_parent.json: what the library of commit 40c1952 returned on an MI355X, when this entry had
    kernels and a host side of its own.  Equality of digests, of the workspace and of the LDS the library asks for."""
    assert_candidates_parents(parent_entries(name, T, dev))
