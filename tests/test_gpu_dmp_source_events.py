"""GPU: source inference from rows of states AND events (gnode_dmp_source_events_scores_f32 through
gnode.dmp.source_scores_events, source_scores_timed and the C entry).

The yardstick is the composition on `dmp_batch`'s float32 marginals from the seed list [c], in numpy: p = Ps, Pi, Pr for the codes
0 / 1 / 2, the float32 differences Ps(t-1) - Ps(t) with Ps(-1) = 1 for code 3 and Pr(t) - Pr(t-1) with Pr(-1) = 0 for code 4, the
float32 clamp to [floor, 1], the float64 logarithm, summed over the coded nodes.  The device forms the same float32 numbers, so
only the rounding of the logarithm and the order of the sum differ, and THE BAR is tests/test_gpu_dmp_source.py's derived one,
    |gpu - ref| <= (n_coded + 4) * 2^-52 * |ref|        (exact equality where ref is 0).
Rows of codes -1 .. 2 are held to `source_scores_batch` with torch.equal.  Which form and which tile serve a graph is asked from
the library."""
import functools
import math

import numpy as np
import pytest

import dmp_grad_model
from baseline_cases import assert_candidates_parents, candidates_entry, er as _er
from sir_cases import dev  # noqa: F401

pytestmark = pytest.mark.gpu

LDS_WORKGROUP = 160 * 1024          # what a gfx950 workgroup may declare
FLOORS = [1e-30, 1e-6]
HORIZONS = [2, 12]                  # 2: no edge pass, and code 3 only on its Ps(0) = ps0 path
NAMES = ["karate", "strided", "general"]
ARG, WORKSPACE = -1, -3             # GNODE_ERR_ARG, GNODE_ERR_WORKSPACE of include/gnode.h
SENTINEL = -12345.0


def _source_lds_bytes(rp, ci):
    from gnode import _lib
    from gnode.graph import DeviceGraph
    return int(_lib.load().gnode_dmp_source_lds_bytes(DeviceGraph(rp, ci).handle))


def _tables(rp, ci, seed):
    """weights 0.5 / mean degree with every 37th raised to 0.9; per-node gamma in [0, 0.6], node 1's exactly 0"""
    n, nnz = len(rp) - 1, len(ci)
    w = np.full(nnz, 0.5 / max(1.0, nnz / n), dtype=np.float32)
    w[::37] = 0.9
    gam = np.random.default_rng(seed).uniform(0.0, 0.6, n).astype(np.float32)
    gam[1] = 0.0
    return w, gam


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(rp, ci, w, gam), read-only.  karate: n 34, one workgroup of 192 threads, no strided loop.  strided: ER on 300 nodes
    with 750 edges and an isolated node 300 appended -- nnz 1 500 > 1 024, so the one workgroup's loops wrap.  general: ER on 700
    nodes (not a multiple of 256: the last block is partial) with 4 400 edges, or as many more as the general form needs.  edge:
    tests/test_gpu_dmp_source.py's 300-node ER graph with one edge fewer, the largest the one-workgroup form serves."""
    if name == "edge":
        from test_gpu_dmp_source import big_er
        rp, ci, _ = _er(300, len(big_er()[1]) // 2 - 1, 40)
    elif name == "karate":
        rp, ci, _ = _er(34, 78, 1)
    elif name == "strided":
        rp, ci, _ = _er(300, 750, 3)
        rp = np.concatenate([rp, rp[-1:]])
    else:
        m = 4400
        rp, ci, _ = _er(700, m, 5)
        while _source_lds_bytes(rp, ci) <= LDS_WORKGROUP:
            m += 200
            rp, ci, _ = _er(700, m, 5)
    w, gam = _tables(rp, ci, 9)
    out = dict(rp=np.asarray(rp), ci=np.asarray(ci), w=w, gam=gam)
    for a in out.values():
        a.setflags(write=False)
    return out


def _n(name):
    return len(case(name)["rp"]) - 1


def cand_list(n):
    """non-contiguous, unsorted, with a repeat (positions 1 and 3); node 1 is the one whose gamma is 0"""
    return (n - 1, 3, n // 2, 3, 0, 1)


@functools.lru_cache(maxsize=None)
def graph(name):
    """one DmpGraph (and so one handle) per case for every call of this file"""
    import scipy.sparse as sp
    from gnode.dmp import DmpGraph
    c, n = case(name), _n(name)
    return DmpGraph(sp.csr_matrix((c["w"].astype(np.float64), c["ci"], c["rp"]), shape=(n, n)))


def coded_rows(name, seeds, codes=(-1, 0, 1, 2, 3, 4), p=(0.2, 0.2, 0.15, 0.15, 0.15, 0.15)):
    n = _n(name)
    return np.stack([np.random.default_rng(100 + int(s)).choice(np.asarray(codes, dtype=np.int8), size=n, p=p) for s in seeds])


def five_logs(out, floor):
    """float64 [5, C, T, n] from `dmp_batch`'s float32 [C, T, n, 3]: the clamped logarithm of every code's probability"""
    ps, pi, pr = (np.ascontiguousarray(out[..., j]) for j in range(3))
    assert ps.dtype == np.float32
    ps_prev = np.concatenate([np.ones_like(ps[:, :1]), ps[:, :-1]], axis=1)
    pr_prev = np.concatenate([np.zeros_like(pr[:, :1]), pr[:, :-1]], axis=1)
    p = np.stack([ps, pi, pr, ps_prev - ps, pr - pr_prev])
    assert p.dtype == np.float32
    return np.log(np.minimum(np.maximum(p, np.float32(floor)), np.float32(1.0)).astype(np.float64))


@functools.lru_cache(maxsize=None)
def reference_logs(name, T, floor):
    """The yardstick's terms for cand_list's candidates, computed once per (case, horizon, floor) and read-only."""
    import torch
    from gnode.dmp import dmp_batch
    out = dmp_batch(graph(name), [[int(k)] for k in cand_list(_n(name))], case(name)["gam"], T)
    assert torch.isfinite(out).all()
    logs = five_logs(out.cpu().numpy(), floor)
    logs.setflags(write=False)
    return logs


def reference(name, T, floor, rows):
    """float64 [R, C, T]: every row's sum over its coded nodes, and the number of coded nodes per row"""
    logs = reference_logs(name, T, floor)
    ref = np.zeros((len(rows),) + logs.shape[1:3])
    for r, row in enumerate(rows):
        for code in range(5):
            ref[r] += logs[code][:, :, row == code].sum(-1)
    return ref, [(int(((row >= 0) & (row <= 4)).sum())) for row in rows]


WORST = {"ratio": 0.0}              # the largest |gpu - ref| / bar this session has seen, printed by every check


def assert_meets_the_bar(got, ref, n_coded, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    for r, count in enumerate(n_coded):
        err, bar = np.abs(got[r] - ref[r]), (count + 4) * 2.0 ** -52 * np.abs(ref[r])
        rel = float(np.max(err / np.maximum(np.abs(ref[r]), 1e-300)))
        WORST["ratio"] = max(WORST["ratio"], rel / ((count + 4) * 2.0 ** -52))
        print(f"{what} row {r}: max |gpu - ref| / |ref| = {rel:.3e}, bar {(count + 4) * 2.0 ** -52:.3e}; worst share of a bar so far {WORST['ratio']:.3f}")
        assert (err <= bar).all(), f"{what} row {r}: {np.max(err - bar):.3e} over the bar"


class EventsEntry:
    """gnode_dmp_source_events_scores_f32 on one graph with device tensors of the caller's making."""

    def __init__(self, name, dev):
        from gnode import _lib
        c = case(name)
        self.lib, self.dev, self.c, self.g = _lib.load(), dev, c, graph(name).graph
        self.w, self.gam = self.up(c["w"]), self.up(c["gam"])

    def tile(self):
        return int(self.lib.gnode_dmp_source_events_tile(self.g.handle))

    def need(self, C, R, T):
        return int(self.lib.gnode_dmp_source_events_workspace_bytes(self.g.handle, C, R, T))

    def one_workgroup(self):
        return int(self.lib.gnode_dmp_source_lds_bytes(self.g.handle)) <= LDS_WORKGROUP

    def up(self, a, dtype=np.float32):
        import torch
        return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(self.dev)       # (a copy: the cases' arrays are read-only)

    def call(self, cand, C, rows, R, floor, T, scores, stride, ws, nbytes=None):
        from gnode import _lib
        return self.lib.gnode_dmp_source_events_scores_f32(self.g.handle, _lib.ptr(self.w), _lib.ptr(self.gam), _lib.ptr(cand), C,
                                                           _lib.ptr(rows), R, floor, T, _lib.ptr(scores), stride, _lib.ptr(ws),
                                                           0 if ws is None else ws.numel() if nbytes is None else nbytes, _lib.stream_ptr())

    def scores(self, cands, rows, T, floor=FLOORS[0]):
        """a served call: the float64 device tensor [R, C, T]"""
        import torch
        C, R = len(cands), len(rows)
        ws = torch.full((self.need(C, R, T),), 0xFF, dtype=torch.uint8, device=self.dev)       # NaNs, should anything read before it writes
        out = torch.full((R, C, T), float("nan"), dtype=torch.float64, device=self.dev)
        rc = self.call(self.up(cands, np.int32), C, self.up(rows, np.int8), R, floor, T, out, C * T, ws)
        assert rc == 0, self.lib.gnode_last_error().decode()
        return out


# ------------------------------------------------------------------ 1. R around the tile, both horizons, both floors
@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("name", NAMES)
def test_rows_of_every_code_meet_the_bar_for_r_around_the_tile(name, T, dev):
    import torch
    from gnode.dmp import source_scores_events
    e = EventsEntry(name, dev)
    assert e.one_workgroup() == (name != "general")
    n, nnz, W = _n(name), len(e.c["ci"]), e.tile()
    assert W >= 1
    if name == "strided":
        assert nnz > 1024 and e.c["rp"][-1] == e.c["rp"][-2] and n == 301                # the loops wrap; the last node is isolated
    if name == "general":
        assert n % 256 != 0 and n > 512
    cands = cand_list(n)
    for R, floor in [(1, FLOORS[0]), (W, FLOORS[0]), (W + 1, FLOORS[0]), (W + 1, FLOORS[1])]:
        rows = coded_rows(name, range(R))
        assert set(np.unique(rows)) <= {-1, 0, 1, 2, 3, 4} and (R < 2 or len(np.unique(rows)) == 6)
        got = source_scores_events(graph(name), rows, e.c["gam"], T, candidates=cands, floor=floor)
        assert got.dtype == torch.float64 and got.shape == (R, len(cands), T)
        ref, counts = reference(name, T, floor, rows)
        assert_meets_the_bar(got.cpu().numpy(), ref, counts, f"{name} T={T} R={R} floor={floor}")
        assert torch.equal(got[:, 1], got[:, 3])                    # the repeated id gives identical tables
        assert torch.equal(got, e.scores(cands, rows, T, floor))    # the C entry on a dirty workspace


# ------------------------------------------------------------------ 2. bit for bit
@pytest.mark.parametrize("name", NAMES)
def test_state_rows_are_source_scores_batch_bit_for_bit(name, dev):
    import torch
    from gnode.dmp import source_scores_batch, source_scores_events
    e = EventsEntry(name, dev)
    W, n, gam, T = e.tile(), _n(name), e.c["gam"], 12
    assert W == int(e.lib.gnode_dmp_source_batch_tile(e.g.handle))
    cands = cand_list(n)
    states = coded_rows(name, range(W + 1), codes=(-1, 0, 1, 2), p=(0.25, 0.35, 0.25, 0.15))
    for floor in FLOORS:
        want = source_scores_batch(graph(name), states, gam, T, candidates=cands, floor=floor)
        assert torch.equal(source_scores_events(graph(name), states, gam, T, candidates=cands, floor=floor), want)
        mixed = coded_rows(name, range(W + 1))
        mixed[W // 2] = states[-1]                                  # a state row among event rows is still the batch entry's row
        assert torch.equal(source_scores_events(graph(name), mixed, gam, T, candidates=cands, floor=floor)[W // 2], want[-1])


@pytest.mark.parametrize("name", NAMES)
def test_a_row_does_not_depend_on_its_company_or_on_the_chunking(name, dev):
    import torch
    from gnode.dmp import source_scores_events
    e = EventsEntry(name, dev)
    W, n, gam, T = e.tile(), _n(name), e.c["gam"], 12
    many = list(cand_list(n))
    rows = coded_rows(name, range(2 * W + 1))
    big = e.scores(many, rows, T)
    assert torch.equal(e.scores(many, rows[3:4], T)[0], big[3])                          # alone
    assert torch.equal(e.scores(many, np.concatenate([rows[W + 2:2 * W + 1], rows[3:4]]), T)[W - 1], big[3])       # the last row of R = W
    other = [many[2], 7, many[0]]                                   # another candidate list, other positions
    got = e.scores(other, rows, T)
    assert torch.equal(got[:, 0], big[:, 2]) and torch.equal(got[:, 2], big[:, 0])
    R = W + 1
    budget = e.need(2, R, T)                                        # two candidates per chunk where the workspace grows with C
    assert (e.need(len(many), R, T) > budget) == (name == "general")                     # six candidates: three chunks
    chunked = source_scores_events(graph(name), rows[:R], gam, T, candidates=many, budget_bytes=budget)        # through score_stride
    assert torch.equal(chunked, big[:R])
    assert torch.equal(source_scores_events(graph(name), rows[:R], gam, T, candidates=many), big[:R])
    with pytest.raises(ValueError):
        source_scores_events(graph(name), rows[:R], gam, T, candidates=many, budget_bytes=e.need(1, R, T) - 1)


def test_the_graph_at_the_lds_edge_keeps_its_form_and_narrows_the_tile(dev):
    import torch
    from gnode.dmp import source_scores_batch, source_scores_events
    e, T = EventsEntry("edge", dev), 12
    W, full = e.tile(), EventsEntry("karate", dev).tile()
    assert e.one_workgroup() and 1 <= W < full and W == int(e.lib.gnode_dmp_source_batch_tile(e.g.handle))
    print(f"the tile at the LDS edge: {W} of {full}")
    assert e.need(1, 3, T) == e.need(50, W + 1, T) > 0              # the one-workgroup form: no room per candidate
    cands = cand_list(_n("edge"))
    for R in (W + 1, 3):
        rows = coded_rows("edge", range(R))
        got = source_scores_events(graph("edge"), rows, e.c["gam"], T, candidates=cands)
        assert_meets_the_bar(got.cpu().numpy(), *reference("edge", T, FLOORS[0], rows), f"edge T={T} R={R}")
    states = coded_rows("edge", range(W + 1), codes=(-1, 0, 1, 2), p=(0.25, 0.35, 0.25, 0.15))
    assert torch.equal(source_scores_events(graph("edge"), states, e.c["gam"], T, candidates=cands),
                       source_scores_batch(graph("edge"), states, e.c["gam"], T, candidates=cands))


# ------------------------------------------------------------------ 3. row 0, and a node that never recovers
@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("name", NAMES)
def test_row_0_and_a_gamma_0_node(name, floor, dev):
    e = EventsEntry(name, dev)
    n, T = _n(name), 12
    cands = cand_list(n)
    log_floor = math.log(float(np.float32(floor)))
    rows = np.full((4, n), -1, dtype=np.int8)
    rows[0, 3] = 3                                                  # "became infected at this step", node 3 alone
    rows[1, 1] = 4                                                  # "recovered at this step", the node whose gamma is 0
    rows[2, [0, 3, n - 1]] = 4                                      # the same of three nodes
    rows[3, 3] = 4
    got = e.scores(cands, rows, T, floor).cpu().numpy()
    for i, k in enumerate(cands):                                   # at t = 0 certain at the candidate itself, at the floor elsewhere
        assert got[0, i, 0] == (0.0 if k == 3 else log_floor), (k, got[0, i, 0])
    assert e.c["gam"][1] == 0.0
    assert (got[1] == log_floor).all()                              # Pr stays 0: at the floor for every candidate and step
    assert (got[3, :, 0] == log_floor).all()                        # nobody recovers at step 0
    assert (np.abs(got[2, :, 0] - 3 * log_floor) <= 7 * 2.0 ** -52 * abs(3 * log_floor)).all()      # log(floor) per coded node
    assert got[3, 1, 1] > log_floor and got[0, 1, 1] == log_floor   # candidate 3 may recover at step 1, and is infected already


# ------------------------------------------------------------------ 4. refusals, and codes that mean nothing
@pytest.mark.parametrize("name", ["karate", "general"])
def test_refusals_leave_scores_untouched_and_other_codes_are_not_observed(name, dev):
    import torch
    e = EventsEntry(name, dev)
    n, T, R = _n(name), 4, 3
    many = cand_list(n)
    C = len(many)
    rows_h = coded_rows(name, range(R))
    rows_h[1, :6] = -1                                              # six nodes that row 1 does not observe, whatever was drawn
    cand, rows = e.up(many, np.int32), e.up(rows_h, np.int8)
    need = e.need(C, R, T)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    scores = torch.full((R, C, T), SENTINEL, dtype=torch.float64, device=dev)
    good = dict(cand=cand, C=C, rows=rows, R=R, floor=FLOORS[0], T=T, scores=scores, stride=C * T, ws=ws)
    for change in (dict(R=0), dict(C=0), dict(T=1), dict(floor=0.0), dict(stride=C * T - 1), dict(R=-2), dict(C=-3), dict(floor=float("nan")),
                   dict(rows=None), dict(cand=None), dict(scores=None), dict(ws=None, nbytes=need)):
        assert e.call(**dict(good, **change)) == ARG, change
    assert e.call(**dict(good, nbytes=need - 1)) == WORKSPACE
    torch.cuda.synchronize()
    assert bool((scores == SENTINEL).all())
    assert e.call(**good) == 0, e.lib.gnode_last_error().decode()
    odd = rows_h.copy()
    hidden = np.flatnonzero(odd[1] == -1)
    assert hidden.size >= 6
    odd[1, hidden] = np.resize(np.asarray([7, -5, 5, -128, 127, -2], dtype=np.int8), hidden.size)       # through the C entry only
    assert torch.equal(e.scores(many, odd, T), scores)              # as if those nodes were -1
    nothing = e.scores(many, np.full((2, n), -1, dtype=np.int8), T)
    assert bool((nothing == 0.0).all()) and not bool(torch.signbit(nothing).any())


# ------------------------------------------------------------------ 5. records taken at different times
@pytest.mark.parametrize("name", NAMES)
def test_timed_scores_are_the_shifted_rows_added_in_order(name, dev):
    import torch
    from gnode.dmp import source_scores_events, source_scores_timed, sum_timed_rows, timed_observations
    e = EventsEntry(name, dev)
    n, T, floor = _n(name), 12, FLOORS[0]
    cands = cand_list(n)
    rng = np.random.default_rng(17)
    nodes = rng.integers(0, n, 40).tolist() + [5, 5, 5, 3]          # node 5 three times at offset -2: three rows there
    offsets = rng.choice([0, -2, -5], 40).tolist() + [-2, -2, -2, 0]
    kinds = rng.integers(0, 5, 40).tolist() + [3, 0, 4, 2]
    obs = timed_observations(n, nodes, offsets, kinds)
    R = len(obs.rows)
    assert sorted(set(obs.row_offsets.tolist())) == [-5, -2, 0] and (obs.row_offsets == -2).sum() >= 3 and obs.row_events.min() >= 0
    got = source_scores_timed(graph(name), obs, e.c["gam"], T, candidates=cands, floor=floor)
    assert got.dtype == torch.float64 and got.shape == (len(cands), T) and got.device.type == dev.type
    table = source_scores_events(graph(name), obs.rows, e.c["gam"], T, candidates=cands, floor=floor)
    assert torch.equal(got, sum_timed_rows(table, obs.row_offsets, obs.row_events, floor))          # its own table, exactly
    ref, counts = reference(name, T, floor, obs.rows)
    before = math.log(float(np.float32(floor)))
    want, bar = np.zeros((len(cands), T)), np.zeros((len(cands), T))
    for r in range(R):
        back = -int(obs.row_offsets[r])
        term = np.full((len(cands), T), int(obs.row_events[r]) * before if obs.row_events[r] else 0.0)
        term[:, back:] = ref[r][:, :T - back]
        slack = np.zeros_like(term)                                 # the pre-outbreak term is the same product on both sides
        slack[:, back:] = (counts[r] + 4) * 2.0 ** -52 * np.abs(ref[r][:, :T - back])
        want, bar = want + term, bar + slack
    err = np.abs(got.cpu().numpy() - want)
    print(f"{name} timed: max |gpu - ref| = {err.max():.3e}, the per-row bars summed there {bar.flat[err.argmax()]:.3e}")
    assert (err <= bar).all()
    default = source_scores_timed(graph(name), obs, e.c["gam"], T, floor=floor)          # every node with a record of a kind != 0
    ids = sorted({k for k, kind in zip(nodes, kinds) if kind != 0})
    assert default.shape == (len(ids), T) and 3 in ids and 5 in ids
    assert torch.equal(default[ids.index(3)], got[1])               # node 3 is cand_list's second


# ------------------------------------------------------------------ 6. end to end
SANITY = dict(n=60, m=150, graph_seed=2, sensor_seed=3, source=17, w=0.35, gamma=0.25, T=24)


def sanity_case():
    """The 60-node connected ER graph, its 12 sensors and, from the float64 model started at the true source, the step at which
    each sensor's onset distribution Ps(t-1) - Ps(t) has its mode: (rp, ci, sensors, onset steps, now)."""
    import torch
    s = SANITY
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    rp, ci, _ = _er(s["n"], s["m"], s["graph_seed"])
    assert connected_components(sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(s["n"], s["n"])))[0] == 1
    src, rev = (torch.from_numpy(a) for a in dmp_grad_model.tables(rp, ci))
    f64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))   # noqa: E731

    def onset(k):                                                   # [T, n]: the probability that a node becomes infected at step t
        out = dmp_grad_model.forward(src, rev, s["n"], f64(np.full(len(ci), s["w"])), f64(np.full(s["n"], s["gamma"])),
                                     f64(dmp_grad_model.seed_state(s["n"], [k])), s["T"])
        ps = out[:, :, 0].numpy()
        return np.concatenate([np.ones((1, s["n"])), ps[:-1]]) - ps
    sensors = np.sort(np.random.default_rng(s["sensor_seed"]).choice(s["n"], 12, replace=False))
    steps = onset(s["source"])[:, sensors].argmax(0)
    return rp, ci, sensors, steps, int(steps.max()), onset


def model_timed_scores(onset, sensors, steps, now, floor=FLOORS[0]):
    """float64 [n, T]: the float64 model's log-likelihood of "sensor j became infected at step steps[j]" when now is t steps after
    candidate c was seeded, with the entry's clamp and its convention for the time before the outbreak"""
    n, T = SANITY["n"], SANITY["T"]
    f = float(np.float32(floor))
    scores = np.zeros((n, T))
    for c in range(n):
        logp = np.log(np.clip(onset(c)[:, sensors], f, 1.0))        # [T, sensors]
        for j, step in enumerate(steps):
            back = now - int(step)
            scores[c, :back] += math.log(f)
            scores[c, back:] += logp[:T - back, j]
    return scores


def test_the_source_is_found_from_twelve_onset_times(dev):
    """The float64 model alone ranks the true source 17 first, 3.07 ahead of the runner-up (node 11), with now = 6 steps after
    the seeding (checked on the CPU when the seeds were chosen, and asserted here again); the device must rank it first too."""
    import scipy.sparse as sp
    from gnode.dmp import observations_from_events, rank_sources, source_scores_timed, timed_observations
    s = SANITY
    rp, ci, sensors, steps, now, onset = sanity_case()
    model = model_timed_scores(onset, sensors, steps, now)
    best = model.max(1)
    order = np.argsort(-best)
    print(f"model: best candidate {order[0]} at t = {model[order[0]].argmax()}, {best[order[0]] - best[order[1]]:.3f} ahead of candidate {order[1]}")
    assert order[0] == s["source"] and best[order[0]] - best[order[1]] >= 1.0
    t_inf = np.full(s["n"], -1)
    t_inf[sensors] = steps
    obs = timed_observations(s["n"], *observations_from_events(t_inf, np.full(s["n"], -1), now, sensors))
    assert obs.row_events.sum() == 12 and obs.row_offsets.min() == -int(now - steps.min())
    A = sp.csr_matrix((np.full(len(ci), s["w"]), ci, rp), shape=(s["n"], s["n"]))
    scores = source_scores_timed(A, obs, s["gamma"], s["T"], candidates=np.arange(s["n"]))
    ranked = rank_sources(scores, np.arange(s["n"]))
    assert ranked[0][0] == s["source"], ranked[:3]


# ------------------------------------------------------------------ 7. the parent's bits
PARENT_CASES = [(name, T) for name in NAMES for T in HORIZONS] + [("edge", 12)]


def parent_entries(name, T, dev):
    """[(key, entry)] of tests/golden/dmp_candidates_parent.json for one case and horizon: R and the floor around the tile as
    test 1 chooses them, and on the graph at the LDS edge that test's two."""
    e = EventsEntry(name, dev)
    W, cands = e.tile(), cand_list(_n(name))
    picks = [(W + 1, FLOORS[0]), (3, FLOORS[0])] if name == "edge" else [(1, FLOORS[0]), (W, FLOORS[0]), (W + 1, FLOORS[0]), (W + 1, FLOORS[1])]
    out = []
    for R, floor in picks:
        sizes = dict(workspace_bytes=e.need(len(cands), R, T), tile=W, lds_bytes=e.lib.gnode_dmp_source_lds_bytes(e.g.handle))
        out.append((f"source_events/{name}/T{T}/R{R}/floor{floor:g}", candidates_entry(e.scores(cands, coded_rows(name, range(R)), T, floor), **sizes)))
    return out


@pytest.mark.parametrize("name,T", PARENT_CASES)
def test_scores_are_the_parents_bits(name, T, dev):
    """tests/golden/dmp_candidates_parent.json: what the library of commit 40c1952 returned on an MI355X, when this entry had
    kernels and a host side of its own.  Equality of digests, of the workspace, of the tile and of the LDS the library asks for."""
    assert_candidates_parents(parent_entries(name, T, dev))
