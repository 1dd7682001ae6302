"""GPU: source inference from many snapshots in one pass (gnode_dmp_source_batch_scores_f32 through gnode.dmp.source_scores_batch
and through the C entry).

The yardstick everywhere is `source_scores` on each row -- the solo entry, which tests/test_gpu_dmp_source.py holds against
`dmp_batch` -- and the comparison is torch.equal: the batch entry promises the solo entry's bits, so there is no tolerance to
choose.  The cases are that file's: er34, isolated and nnz0 are served by the one-workgroup form, hub and big_er (n = 300: two
blocks per candidate, so the partial add runs) by the general form.  Which form and which tile serve a graph is asked from the
library, not restated here."""
import functools

import numpy as np
import pytest

import dmp_grad_model
from baseline_cases import assert_candidates_parents, candidates_entry, er as _er
from sir_cases import dev  # noqa: F401
from test_gpu_dmp_source import big_er, cand_list, case, mixed_obs

pytestmark = pytest.mark.gpu

LDS_WORKGROUP = 160 * 1024          # what a gfx950 workgroup may declare
FLOOR = 1e-30
HORIZONS = [2, 8]                   # 2: no edge pass at all
N_BIG = 300
ONE_WORKGROUP, GENERAL = ["er34", "isolated", "nnz0"], ["hub", "big_er"]
FORM_CASE = {"one_workgroup": "er34", "general": "big_er"}
ARG, WORKSPACE = -1, -3             # GNODE_ERR_ARG, GNODE_ERR_WORKSPACE of include/gnode.h
SENTINEL = -12345.0


@functools.lru_cache(maxsize=None)
def edge_case():
    """`big_er()`'s graph with one edge fewer, the largest the solo one-workgroup form serves, with big_er's kind of tables."""
    m = len(big_er()[1]) // 2                                       # er's graphs have exactly m undirected edges
    rp, ci, _ = _er(N_BIG, m - 1, 40)
    s = 5.0 * N_BIG / len(ci)
    out = dict(rp=np.asarray(rp), ci=np.asarray(ci), w=np.asarray(dmp_grad_model.weights(len(ci), 0.05 * s, 0.4 * s, 21), np.float32),
               gam=np.asarray(dmp_grad_model.gammas(N_BIG, 22), np.float32))
    assert not (out["w"] == 1.0).any()
    for a in out.values():
        a.setflags(write=False)
    return out


def _case(name):
    return edge_case() if name == "edge" else case(name)


def _n(name):
    return len(_case(name)["rp"]) - 1


@functools.lru_cache(maxsize=None)
def graph(name):
    """one DmpGraph (and so one handle) per case for every Python-surface call of this file"""
    import scipy.sparse as sp
    from gnode.dmp import DmpGraph
    c, n = _case(name), _n(name)
    return DmpGraph(sp.csr_matrix((c["w"].astype(np.float64), c["ci"], c["rp"]), shape=(n, n)))


def rows(name, seeds):
    return np.stack([mixed_obs(_n(name), seed=int(s)) for s in seeds]).astype(np.int8)


@functools.lru_cache(maxsize=None)
def solo(name, T, seed, cands):
    """The yardstick: `source_scores` of the snapshot mixed_obs(n, seed) alone, computed once; a float64 device tensor [C, T]
    that no test writes to."""
    from gnode.dmp import source_scores
    return source_scores(graph(name), mixed_obs(_n(name), seed=seed), _case(name)["gam"], T, candidates=list(cands), floor=FLOOR)


def solo_table(name, T, seeds, cands):
    import torch
    return torch.stack([solo(name, T, int(s), tuple(cands)) for s in seeds])


class BatchEntry:
    """gnode_dmp_source_batch_scores_f32 on one graph with device tensors of the caller's making."""

    def __init__(self, name, dev):
        from gnode import _lib
        c = _case(name)
        self.lib, self.dev, self.c, self.g = _lib.load(), dev, c, graph(name).graph
        self.w, self.gam = self.up(c["w"]), self.up(c["gam"])

    def tile(self):
        return int(self.lib.gnode_dmp_source_batch_tile(self.g.handle))

    def need(self, C, O, T):
        return int(self.lib.gnode_dmp_source_batch_workspace_bytes(self.g.handle, C, O, T))

    def one_workgroup(self):
        return int(self.lib.gnode_dmp_source_lds_bytes(self.g.handle)) <= LDS_WORKGROUP

    def up(self, a, dtype=np.float32):
        import torch
        a = np.array(a, dtype=dtype, order="C")                     # (a copy: the cases' arrays are read-only)
        return None if a.size == 0 else torch.from_numpy(a).to(self.dev)       # (no edge, no table)

    def call(self, cand, C, obs, O, floor, T, scores, stride, ws, nbytes=None):
        from gnode import _lib
        return self.lib.gnode_dmp_source_batch_scores_f32(self.g.handle, _lib.ptr(self.w), _lib.ptr(self.gam), _lib.ptr(cand), C, _lib.ptr(obs),
                                                          O, floor, T, _lib.ptr(scores), stride, _lib.ptr(ws),
                                                          0 if ws is None else ws.numel() if nbytes is None else nbytes, _lib.stream_ptr())

    def scores(self, cands, obs, T, ws=None):
        """a served call: the float64 device tensor [O, C, T]"""
        import torch
        C, O = len(cands), len(obs)
        ws = torch.empty(self.need(C, O, T), dtype=torch.uint8, device=self.dev) if ws is None else ws
        out = torch.full((O, C, T), float("nan"), dtype=torch.float64, device=self.dev)
        rc = self.call(self.up(cands, np.int32), C, self.up(obs, np.int8), O, FLOOR, T, out, C * T, ws)
        assert rc == 0, self.lib.gnode_last_error().decode()
        return out


def full_tile(dev):
    return BatchEntry("er34", dev).tile()


# ------------------------------------------------------------------ 1. O around the tile
@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("name", ONE_WORKGROUP + GENERAL)
def test_every_row_is_the_solo_table_for_o_around_the_tile(name, T, dev):
    import torch
    from gnode.dmp import source_scores_batch
    e = BatchEntry(name, dev)
    assert e.one_workgroup() == (name in ONE_WORKGROUP)
    W = e.tile()
    assert W >= 1
    cands = cand_list(_n(name))
    for O in sorted({o for o in (1, W - 1, W, W + 1, 2 * W + 1) if o >= 1}):
        got = source_scores_batch(graph(name), rows(name, range(O)), e.c["gam"], T, candidates=cands, floor=FLOOR)
        assert got.dtype == torch.float64 and got.shape == (O, len(cands), T)
        want = solo_table(name, T, range(O), cands)
        same = [bool(torch.equal(got[o], want[o])) for o in range(O)]
        assert all(same), f"{name} T={T} O={O} W={W}: rows {[o for o in range(O) if not same[o]]} differ from the solo call"


# ------------------------------------------------------------------ 2. a row does not depend on its company
@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_a_row_does_not_depend_on_its_company(form, dev):
    import torch
    from gnode.dmp import source_scores_batch
    name, T = FORM_CASE[form], 8
    e = BatchEntry(name, dev)
    W, n, gam = e.tile(), _n(name), e.c["gam"]
    many = list(cand_list(n))
    big = e.scores(many, rows(name, range(2 * W + 1)), T)
    assert torch.equal(e.scores(many, rows(name, [3]), T)[0], big[3])                    # row 0 of O = 1
    assert torch.equal(e.scores(many, rows(name, list(range(100, 100 + W - 1)) + [3]), T)[W - 1], big[3])       # the last row of O = W
    other = [many[2], 7, many[0]]                                   # another candidate list, other positions
    got = e.scores(other, rows(name, range(2 * W + 1)), T)
    assert torch.equal(got[:, 0], big[:, 2]) and torch.equal(got[:, 2], big[:, 0])
    O = W + 1
    budget = e.need(2, O, T)                                        # two candidates per chunk where the workspace grows with C
    assert (e.need(len(many), O, T) > budget) == (form == "general")          # five candidates: three chunks
    obs = rows(name, range(O))
    chunked = source_scores_batch(graph(name), obs, gam, T, candidates=many, floor=FLOOR, budget_bytes=budget)      # through score_stride
    assert torch.equal(chunked, big[:O])
    assert torch.equal(source_scores_batch(graph(name), obs, gam, T, candidates=many, floor=FLOOR), big[:O])
    with pytest.raises(ValueError):
        source_scores_batch(graph(name), obs, gam, T, candidates=many, budget_bytes=e.need(1, O, T) - 1)


# ------------------------------------------------------------------ 3. the graph at the LDS edge
def test_the_graph_at_the_lds_edge_keeps_its_form_and_narrows_the_tile(dev):
    import torch
    from gnode.dmp import source_scores_batch
    e, W, T = BatchEntry("edge", dev), full_tile(dev), 8
    assert int(e.lib.gnode_dmp_source_lds_bytes(e.g.handle)) == big_er()[3] <= LDS_WORKGROUP < big_er()[2]
    assert 1 <= e.tile() <= W
    print(f"the tile at the LDS edge: {e.tile()} of {W}")
    assert e.need(1, 3, T) == e.need(50, 3, T) == e.need(50, W + 1, T) > 0              # the one-workgroup form: no room per candidate
    cands = cand_list(N_BIG)
    for O in (3, W + 1):
        got = source_scores_batch(graph("edge"), rows("edge", range(O)), e.c["gam"], T, candidates=cands, floor=FLOOR)
        assert torch.equal(got, solo_table("edge", T, range(O), cands)), O


# ------------------------------------------------------------------ 4. not observed means nothing
@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_not_observed_means_nothing(form, dev):
    import torch
    name, T = FORM_CASE[form], 8
    e = BatchEntry(name, dev)
    n, cands = _n(name), cand_list(_n(name))
    obs = rows(name, range(3))
    obs[1] = -1                                                     # nothing observed, between two rows that are
    got = e.scores(cands, obs, T)
    assert bool((got[1] == 0.0).all()) and not bool(torch.signbit(got[1]).any())
    assert float(got[0].max()) < 0.0 and float(got[2].max()) < 0.0
    assert torch.equal(got[0], solo(name, T, 0, tuple(cands))) and torch.equal(got[2], solo(name, T, 2, tuple(cands)))
    odd = rows(name, range(3))
    hidden = np.flatnonzero(odd[1] == -1)
    assert hidden.size >= 4
    odd[1, hidden] = np.resize(np.asarray([7, -5, 3, -128, 127, -2], dtype=np.int8), hidden.size)     # through the C entry only
    assert torch.equal(e.scores(cands, odd, T)[1], solo(name, T, 1, tuple(cands)))       # as if those nodes were -1


# ------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_refusals_leave_scores_untouched_and_a_good_call_is_served(form, dev):
    import torch
    name, T, O = FORM_CASE[form], 4, 3
    e = BatchEntry(name, dev)
    many = cand_list(_n(name))
    C = len(many)
    cand, obs = e.up(many, np.int32), e.up(rows(name, range(O)), np.int8)
    need = e.need(C, O, T)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    scores = torch.full((O, C, T), SENTINEL, dtype=torch.float64, device=dev)
    good = dict(cand=cand, C=C, obs=obs, O=O, floor=FLOOR, T=T, scores=scores, stride=C * T, ws=ws)
    for change in (dict(O=0), dict(C=0), dict(T=1), dict(floor=0.0), dict(stride=C * T - 1), dict(O=-2), dict(C=-3), dict(floor=float("nan")),
                   dict(obs=None), dict(cand=None), dict(scores=None), dict(ws=None, nbytes=need)):
        assert e.call(**dict(good, **change)) == ARG, change
    assert e.call(**dict(good, nbytes=need - 1)) == WORKSPACE
    torch.cuda.synchronize()
    assert bool((scores == SENTINEL).all())
    assert e.call(**good) == 0, e.lib.gnode_last_error().decode()
    assert torch.equal(scores, solo_table(name, T, range(O), many))


# ------------------------------------------------------------------ 6. the device-tensor path
def test_a_device_table_of_snapshots_is_scored_where_it_lies(dev):
    import torch
    from gnode.dmp import source_scores_batch
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import sir_state_at, sir_trajectories
    c, T = case("er34"), 8
    traj = sir_trajectories(DeviceGraph(c["rp"], c["ci"]), [5], 0.4, 0.3, sims=6, T=10, rng_seed=11, curves=False)
    state = sir_state_at(traj.t_inf, traj.t_rec, 4)
    assert state.is_cuda and state.dtype == torch.int8 and state.shape == (6, 34)
    assert int(state.min()) >= 0 and int(state.max()) <= 2 and bool((state[:, 5] >= 1).all())
    got = source_scores_batch(graph("er34"), state, c["gam"], T)
    host = source_scores_batch(graph("er34"), state.cpu().numpy(), c["gam"], T)
    assert got.shape == host.shape and got.shape[0] == 6 and got.shape[2] == T and torch.equal(got, host)
    assert torch.equal(source_scores_batch(graph("er34"), state.to(torch.int64), c["gam"], T), host)
    bad = state.clone()
    bad[2, 7] = 3
    for table in (bad, bad[:, :-1], bad[0], bad[:0]):
        with pytest.raises(ValueError):
            source_scores_batch(graph("er34"), table, c["gam"], T)


# ------------------------------------------------------------------ 7. end to end
def test_the_sources_of_three_path_outbreaks_are_found(dev):
    """The 9-node path of test_gpu_dmp_source.py's last test (weights 0.5, gamma 0.3, maxTime 8) with three snapshots built
    the way that test builds its one: the source recovered, its two neighbours infected, the rest susceptible."""
    import scipy.sparse as sp
    from gnode.dmp import source_rank_of, source_scores_batch
    n, T, truth = 9, 8, [2, 4, 6]
    rp = np.concatenate([[0], np.cumsum([1] + [2] * (n - 2) + [1])]).astype(np.int32)
    ci = np.asarray([j for i in range(n) for j in (i - 1, i + 1) if 0 <= j < n], dtype=np.int32)
    A = sp.csr_matrix((np.full(len(ci), 0.5), ci, rp), shape=(n, n))
    obs = np.zeros((3, n), dtype=np.int64)
    for o, s in enumerate(truth):
        obs[o, [s - 1, s + 1]], obs[o, s] = 1, 2
    scores = source_scores_batch(A, obs, 0.3, T, candidates=np.arange(n))
    assert scores.shape == (3, n, T)
    assert source_rank_of(scores, np.arange(n), truth).tolist() == [0, 0, 0]
    assert source_rank_of(scores.cpu().numpy(), np.arange(n), truth).tolist() == [0, 0, 0]
    assert source_rank_of(scores, np.arange(n), [4, 2, 2]).min().item() > 0              # a wrong guess is not ranked first


# ------------------------------------------------------------------ 8. reproducible
@pytest.mark.parametrize("form", ["one_workgroup", "general"])
def test_reproducible_on_a_dirty_workspace(form, dev):
    import torch
    name, T = FORM_CASE[form], 8
    e = BatchEntry(name, dev)
    many = list(cand_list(_n(name)))
    O = e.tile() + 1
    obs = rows(name, range(O))
    ws = torch.full((e.need(len(many), O + 2, T + 1),), 0xFF, dtype=torch.uint8, device=dev)      # NaNs, should anything read before it writes
    first = e.scores(many, obs, T, ws=ws)
    e.scores(many[:3], rows(name, range(50, 52 + O)), T + 1, ws=ws)                      # a larger call, other numbers
    assert torch.equal(e.scores(many, obs, T, ws=ws), first)
    assert torch.equal(first, solo_table(name, T, range(O), many))


# ------------------------------------------------------------------ 9. the parent's bits
PARENT_CASES = [(name, T) for name in ONE_WORKGROUP + GENERAL for T in HORIZONS] + [("edge", 8)]


def parent_entries(name, T, dev):
    """[(key, entry)] of tests/golden/dmp_candidates_parent.json for one case and horizon: O around the tile as test 1 chooses
    it, and on the graph at the LDS edge test 3's two."""
    e = BatchEntry(name, dev)
    W, cands = e.tile(), cand_list(_n(name))
    out = []
    for O in (3, W + 1) if name == "edge" else sorted({o for o in (1, W - 1, W, W + 1, 2 * W + 1) if o >= 1}):
        sizes = dict(workspace_bytes=e.need(len(cands), O, T), tile=W, lds_bytes=e.lib.gnode_dmp_source_lds_bytes(e.g.handle))
        out.append((f"source_batch/{name}/T{T}/O{O}", candidates_entry(e.scores(cands, rows(name, range(O)), T), **sizes)))
    return out


@pytest.mark.parametrize("name,T", PARENT_CASES)
def test_scores_are_the_parents_bits(name, T, dev):
    """tests/golden/dmp_candidates_parent.json: what the library of commit 40c1952 returned on an MI355X, when this entry had
    kernels and a host side of its own.  Equality of digests, of the workspace, of the tile and of the LDS the library asks for."""
    assert_candidates_parents(parent_entries(name, T, dev))
