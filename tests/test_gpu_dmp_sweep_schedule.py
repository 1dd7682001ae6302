"""GPU: source scores and outbreak sizes under a rate schedule (gnode_dmp_source_events_scores_schedule_f32 and
gnode_dmp_outbreak_sizes_schedule_f32 through gnode.dmp.source_scores_schedule, outbreak_sizes_schedule and the C entries).

A sample is a candidate and a SHIFT: step t of its run is governed by phase[shift + t].  The yardstick is the existing `dmp_batch`
under `rate_schedule(values, steps=` the phase row from the shift on `)`, which tests/test_gpu_dmp_schedule.py pins, from the
seed list [c] (scores) or from the base start with the candidate's row replaced (sizes), composed in numpy: `five_logs` summed
over a row's coded nodes, and (marginals * value) summed over the nodes.  The device forms the same float32 marginals, so THE
BARS are the derived ones of tests/test_gpu_dmp_source_events.py and tests/test_gpu_dmp_outbreak.py,
    scores   |gpu - ref| <= (n_coded + 4) * 2^-52 * |ref|
    sizes    |gpu - ref| <= n * 2^-52 * sum_k |value_k * P^k_j|.
The graphs, rows and candidates are tests/test_gpu_dmp_source_events.py's; which form and tile serve a graph is asked from the
library."""
import functools

import numpy as np
import pytest

import dmp_grad_model
import dmp_sweep_schedule_model as M
from sir_cases import dev  # noqa: F401
from test_gpu_dmp_outbreak import starts_of
from test_gpu_dmp_source_events import assert_meets_the_bar, cand_list, case, coded_rows, five_logs, graph

pytestmark = pytest.mark.gpu

NAMES = ["karate", "strided", "general"]
HORIZONS = [2, 3, 12]               # 2: no edge pass, only phase[shift + 1] is read; 3: one edge pass, whose w_next is the last valid entry
ACTIONS = {"seed": 0, "immunise": 1}
ARG, WORKSPACE = -1, -3             # GNODE_ERR_ARG, GNODE_ERR_WORKSPACE of include/gnode.h
SENTINEL = -12345.0
FLOOR = 1e-30
# L = 17; entry 0 is never read.  It changes between steps 1 and 2, revisits phase 0, and changes at the last step of the
# windows that the shifts 0, 1 and L - T open for T = 12 (entries 11, 12, 16) and of the shifts 0 and L - T for T = 3 (2, 16).
PHASE = np.asarray([0, 0, 1, 1, 1, 2, 2, 0, 0, 1, 1, 2, 0, 1, 1, 0, 2], dtype=np.int32)
L = len(PHASE)
PHASE.setflags(write=False)


def test_the_phase_row_is_what_the_cases_need():
    assert L == 17 and PHASE[1] != PHASE[2] and (PHASE[7:9] == 0).all() and PHASE[6] != 0 and set(PHASE[1:].tolist()) == {0, 1, 2}
    for T, shifts in ((12, (0, 1, L - 12)), (3, (0, L - 3))):
        for s in shifts:
            assert PHASE[s + T - 1] != PHASE[s + T - 2], (T, s)


def _n(name):
    return len(case(name)["rp"]) - 1


@functools.lru_cache(maxsize=None)
def tables(name):
    """(W float32 [3, nnz], G float32 [3, n]), read-only: open, a quarter of the contacts, closed but for the 0.9 entries; gamma,
    2.5 gamma capped at 1, gamma"""
    w, gam = case(name)["w"], case(name)["gam"]
    W = np.stack([w, (w.astype(np.float64) * 0.25).astype(np.float32), np.where(w == np.float32(0.9), w, np.float32(0.0))]).astype(np.float32)
    G = np.stack([gam, np.minimum(np.float32(2.5) * gam, np.float32(1.0)), gam]).astype(np.float32)
    assert (W[2] > 0).any() and (W[2] == 0).any()
    W.setflags(write=False); G.setflags(write=False)
    return W, G


def matrices(name, W=None):
    import scipy.sparse as sp
    c, n = case(name), _n(name)
    return [sp.csr_matrix((w.astype(np.float64), c["ci"], c["rp"]), shape=(n, n)) for w in (tables(name)[0] if W is None else W)]


def samples(name, T):
    """(ids, shifts): cand_list's candidates -- node 3 twice -- with the shifts 0, 1 and L - T; node 3's two samples share the
    shift 1, and it comes a third time, last, with the shift 0"""
    ids = list(cand_list(_n(name))) + [3]
    return ids, [0, 1, L - T, 1, L - T, 0, 0]


def moved(row, s, T):
    return np.ascontiguousarray(np.asarray(row)[s:s + T])


def batch_under(name, starts_by_sample, shifts, T, phase=PHASE):
    """float32 [C, T, n, 3] on the host: `dmp_batch` of every sample's start under the phase row moved by its shift, one call per
    distinct shift"""
    from gnode.dmp import dmp_batch
    from gnode.ode_nn import rate_schedule
    import torch
    out = [None] * len(shifts)
    for s in sorted(set(shifts)):
        at = [j for j, x in enumerate(shifts) if x == s]
        row = moved(phase, s, T)
        got = dmp_batch(rate_schedule(matrices(name), steps=row), [starts_by_sample[j] for j in at], rate_schedule(list(tables(name)[1]), steps=row), T)
        assert torch.isfinite(got).all()
        for j, o in zip(at, got.cpu().numpy()):
            out[j] = o
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def reference_logs(name, T):
    ids, shifts = samples(name, T)
    logs = five_logs(batch_under(name, [[int(k)] for k in ids], shifts, T), FLOOR)
    logs.setflags(write=False)
    return logs


def reference_scores(name, T, rows):
    logs = reference_logs(name, T)
    ref = np.zeros((len(rows),) + logs.shape[1:3])
    for r, row in enumerate(rows):
        for code in range(5):
            ref[r] += logs[code][:, :, row == code].sum(-1)
    return ref, [int(((row >= 0) & (row <= 4)).sum()) for row in rows]


@functools.lru_cache(maxsize=None)
def base_start(name):
    p = np.ascontiguousarray(dmp_grad_model.mixed_state(_n(name), 50), dtype=np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def values(name):
    rng = np.random.default_rng(7)
    v = rng.uniform(0.0, 3.0, _n(name)).astype(np.float32)
    v[rng.random(_n(name)) < 0.1] = 0.0
    v.setflags(write=False)
    return v


def outbreak_samples(name, T):
    """`samples` with a "no change" run, -1, at shift 1 behind them"""
    ids, shifts = samples(name, T)
    return ids + [-1], shifts + [1]


@functools.lru_cache(maxsize=None)
def reference_marginals(name, T, action):
    ids, shifts = outbreak_samples(name, T)
    out = batch_under(name, starts_of(base_start(name), ids, action), shifts, T)
    out.setflags(write=False)
    return out


def reference_sizes(name, T, action, valued):
    out = reference_marginals(name, T, action).astype(np.float64)
    v = (values(name) if valued else np.ones(_n(name), dtype=np.float32)).astype(np.float64)[None, None, :, None]
    return (out * v).sum(2), (np.abs(out) * v).sum(2)


def assert_sizes_meet_the_bar(got, ref, mag, n, what):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err, bar = np.abs(got - ref), n * 2.0 ** -52 * mag
    print(f"{what}: max |gpu - ref| / sum |term| = {float(np.max(err / np.maximum(mag, 1e-300))):.3e}, bar {n * 2.0 ** -52:.3e}")
    assert (err <= bar).all(), f"{what}: {np.max(err - bar):.3e} over the bar"


class Entries:
    """The two C entries on one graph, with device tensors of the caller's making and a workspace filled with 0xFF."""

    def __init__(self, name, dev, W=None, G=None):
        from gnode import _lib
        self.lib, self.dev, self.name, self.g = _lib.load(), dev, name, graph(name).graph
        W, G = (tables(name)[0] if W is None else W), (tables(name)[1] if G is None else G)
        self.P, self.W, self.G = len(G), self.up(W), self.up(G)
        self.base, self.value = self.up(base_start(name)), self.up(values(name))

    def up(self, a, dtype=np.float32):
        import torch
        return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(self.dev)

    def tile(self):
        return int(self.lib.gnode_dmp_source_events_tile(self.g.handle))

    def one_workgroup(self):
        return int(self.lib.gnode_dmp_source_lds_bytes(self.g.handle)) <= 160 * 1024

    def need_scores(self, C, R, T, rows_L=L):
        return int(self.lib.gnode_dmp_source_events_schedule_workspace_bytes(self.g.handle, C, R, T, rows_L))

    def need_sizes(self, C, T, rows_L=L):
        return int(self.lib.gnode_dmp_outbreak_schedule_workspace_bytes(self.g.handle, C, T, rows_L))

    def call_scores(self, cand, shifts, C, rows, R, T, scores, stride, ws, phase=PHASE, P=None, rows_L=None, floor=FLOOR, nbytes=None, W="own", G="own"):
        from gnode import _lib
        ph = None if phase is None else np.ascontiguousarray(phase, dtype=np.int32)
        sh = None if shifts is None else np.ascontiguousarray(shifts, dtype=np.int32)
        return self.lib.gnode_dmp_source_events_scores_schedule_f32(
            self.g.handle, _lib.ptr(self.W if isinstance(W, str) else W), _lib.ptr(self.G if isinstance(G, str) else G),
            None if ph is None else _lib.host_ptr(ph), self.P if P is None else P, (0 if ph is None else len(ph)) if rows_L is None else rows_L,
            _lib.ptr(cand), None if sh is None else _lib.host_ptr(sh), C, _lib.ptr(rows), R, floor, T, _lib.ptr(scores), stride, _lib.ptr(ws),
            0 if ws is None else ws.numel() if nbytes is None else nbytes, _lib.stream_ptr())

    def call_sizes(self, cand, shifts, C, action, value, T, sizes, ws, phase=PHASE, P=None, rows_L=None, nbytes=None, init="own", W="own", G="own"):
        from gnode import _lib
        ph = None if phase is None else np.ascontiguousarray(phase, dtype=np.int32)
        sh = None if shifts is None else np.ascontiguousarray(shifts, dtype=np.int32)
        return self.lib.gnode_dmp_outbreak_sizes_schedule_f32(
            self.g.handle, _lib.ptr(self.W if isinstance(W, str) else W), _lib.ptr(self.G if isinstance(G, str) else G),
            None if ph is None else _lib.host_ptr(ph), self.P if P is None else P, (0 if ph is None else len(ph)) if rows_L is None else rows_L,
            _lib.ptr(self.base if isinstance(init, str) else init), _lib.ptr(cand), None if sh is None else _lib.host_ptr(sh), C, action,
            _lib.ptr(value), T, _lib.ptr(sizes), _lib.ptr(ws), 0 if ws is None else ws.numel() if nbytes is None else nbytes, _lib.stream_ptr())

    def scores(self, ids, shifts, rows, T, phase=PHASE):
        """a served call: the float64 device tensor [R, C, T]"""
        import torch
        C, R = len(ids), len(rows)
        ws = torch.full((self.need_scores(C, R, T, len(phase)),), 0xFF, dtype=torch.uint8, device=self.dev)
        out = torch.full((R, C, T), float("nan"), dtype=torch.float64, device=self.dev)
        rc = self.call_scores(self.up(ids, np.int32), shifts, C, self.up(rows, np.int8), R, T, out, C * T, ws, phase=phase)
        assert rc == 0, self.lib.gnode_last_error().decode()
        return out

    def sizes(self, ids, shifts, T, action, valued, phase=PHASE):
        """a served call: the float64 device tensor [C, T, 3]"""
        import torch
        C = len(ids)
        ws = torch.full((self.need_sizes(C, T, len(phase)),), 0xFF, dtype=torch.uint8, device=self.dev)
        out = torch.full((C, T, 3), float("nan"), dtype=torch.float64, device=self.dev)
        rc = self.call_sizes(self.up(ids, np.int32), shifts, C, ACTIONS[action], self.value if valued else None, T, out, ws, phase=phase)
        assert rc == 0, self.lib.gnode_last_error().decode()
        return out


def schedules(name, row, W=None, G=None):
    """(weight_adj, gamma) as RateSchedules over the phase row, for the Python calls"""
    from gnode.ode_nn import rate_schedule
    return rate_schedule(matrices(name, W), steps=row), rate_schedule(list(tables(name)[1] if G is None else G), steps=row)


# ------------------------------------------------------------------ 1. the bars: every case, horizon, shift, action, value, R
@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("name", NAMES)
def test_scores_and_sizes_meet_their_bars(name, T, dev):
    import torch
    e = Entries(name, dev)
    assert e.one_workgroup() == (name != "general")
    n, W = _n(name), e.tile()
    ids, shifts = samples(name, T)
    assert set(shifts) == {0, 1, L - T} and ids[1] == ids[3] == ids[6] and shifts[1] == shifts[3] != shifts[6]
    assert case(name)["rp"][4] > case(name)["rp"][3]               # node 3 has neighbours: the weights matter to its runs
    for R in (1, W, W + 1):
        rows = coded_rows(name, range(R))
        got = e.scores(ids, shifts, rows, T)
        assert got.dtype == torch.float64 and got.shape == (R, len(ids), T)
        ref, counts = reference_scores(name, T, rows)
        assert_meets_the_bar(got.cpu().numpy(), ref, counts, f"{name} T={T} R={R}")
        assert torch.equal(got[:, 1], got[:, 3])                    # the two identical samples
        if T > 2:
            assert not torch.equal(got[:, 1], got[:, 6])            # one candidate, two shifts: the schedule matters
    oids, oshifts = outbreak_samples(name, T)
    for action in ACTIONS:
        for valued in (False, True):
            got = e.sizes(oids, oshifts, T, action, valued)
            assert_sizes_meet_the_bar(got.cpu().numpy(), *reference_sizes(name, T, action, valued), n, f"{name} T={T} {action} valued={valued}")
            assert torch.equal(got[1], got[3])


# ------------------------------------------------------------------ 2. a schedule that changes nothing: the constant entries' bits
@pytest.mark.parametrize("name", NAMES)
def test_a_schedule_that_changes_nothing_gives_the_constant_entries_bits(name, dev):
    import torch
    from gnode.dmp import outbreak_sizes, outbreak_sizes_schedule, source_scores_events, source_scores_schedule
    from gnode.ode_nn import initial_state
    T, c = 12, case(name)
    ids, shifts = samples(name, T)
    oids, oshifts = outbreak_samples(name, T)
    rows = coded_rows(name, range(Entries(name, dev).tile() + 1))
    want = source_scores_events(graph(name), rows, c["gam"], T, candidates=ids)
    start = initial_state(base_start(name).astype(np.float64))
    want_sizes = {(a, v): outbreak_sizes(graph(name), c["gam"], T, candidates=oids, action=a, start=start, value=values(name) if v else None)
                  for a in ACTIONS for v in (False, True)}
    one = Entries(name, dev, W=c["w"][None], G=c["gam"][None])                            # one phase
    same = Entries(name, dev, W=np.stack([c["w"]] * 3), G=np.stack([c["gam"]] * 3))       # three phases of equal tables
    for e, phase, sh, osh in ((one, np.zeros(L, dtype=np.int32), shifts, oshifts), (one, np.zeros(T, dtype=np.int32), None, None),
                              (same, PHASE, shifts, oshifts)):
        assert torch.equal(e.scores(ids, sh, rows, T, phase=phase), want)
        for (a, v), w_ in want_sizes.items():
            assert torch.equal(e.sizes(oids, osh, T, a, v, phase=phase), w_)
    # the Python calls without any schedule, and with one of equal values
    assert torch.equal(source_scores_schedule(graph(name), rows, c["gam"], T, candidates=ids), want)
    wa, ga = schedules(name, PHASE, W=[c["w"]] * 3, G=[c["gam"]] * 3)
    assert torch.equal(source_scores_schedule(wa, rows, ga, T, candidates=ids, observed_at=L - 1), want)
    assert torch.equal(outbreak_sizes_schedule(wa, ga, T, candidates=oids, action="immunise", start=start, value=values(name), shifts=oshifts),
                       want_sizes[("immunise", True)])


# ------------------------------------------------------------------ 3. the shift is a move of the row; company, position, chunking
@pytest.mark.parametrize("name", NAMES)
def test_a_shift_moves_the_row_and_a_sample_does_not_depend_on_its_company(name, dev):
    import torch
    from gnode.dmp import outbreak_sizes_schedule, source_scores_schedule
    from gnode.ode_nn import initial_state
    e, T = Entries(name, dev), 12
    ids, shifts = samples(name, T)
    oids, oshifts = outbreak_samples(name, T)
    rows = coded_rows(name, range(e.tile() + 1))
    big, big_sizes = e.scores(ids, shifts, rows, T), e.sizes(oids, oshifts, T, "seed", True)
    for j in (0, 2, 6):                                             # (c, shift s) under the row = (c, shift 0) under the row moved by s
        assert torch.equal(e.scores([ids[j]], [0], rows, T, phase=moved(PHASE, shifts[j], T))[:, 0], big[:, j])
        assert torch.equal(e.scores([ids[j]], None, rows, T, phase=moved(PHASE, shifts[j], L))[:, 0], big[:, j])      # null shifts: all 0
        assert torch.equal(e.sizes([oids[j]], [0], T, "seed", True, phase=moved(PHASE, oshifts[j], T))[0], big_sizes[j])
    back = list(range(len(ids)))[::-1]                              # other positions, other company
    assert torch.equal(e.scores([ids[j] for j in back], [shifts[j] for j in back], rows, T), big[:, back])
    assert torch.equal(e.scores(ids[2:5], shifts[2:5], rows[1:2], T)[0], big[1, 2:5])
    oback = list(range(len(oids)))[::-1]
    assert torch.equal(e.sizes([oids[j] for j in oback], [oshifts[j] for j in oback], T, "seed", True), big_sizes[oback])
    # the Python calls and their chunking: two samples per chunk where the workspace grows with the samples
    wa, ga = schedules(name, PHASE)
    start = initial_state(base_start(name).astype(np.float64))
    py_sizes = outbreak_sizes_schedule(wa, ga, T, candidates=oids, action="seed", start=start, value=values(name), shifts=oshifts)
    assert torch.equal(py_sizes, big_sizes)                         # the C entry on a dirty workspace returns the Python call's bits
    budget = e.need_sizes(2, T, max(oshifts) + T)
    assert (e.need_sizes(len(oids), T, max(oshifts) + T) > budget) == (name == "general")
    assert torch.equal(outbreak_sizes_schedule(wa, ga, T, candidates=oids, action="seed", start=start, value=values(name), shifts=oshifts,
                                               budget_bytes=budget), big_sizes)
    zero = source_scores_schedule(wa, rows, ga, T, candidates=ids)                        # observed_at=None: shift 0 for everybody
    assert torch.equal(zero, e.scores(ids, [0] * len(ids), rows, T))
    assert torch.equal(source_scores_schedule(wa, rows, ga, T, candidates=ids, budget_bytes=e.need_scores(2, len(rows), T, T)), zero)
    with pytest.raises(ValueError):
        source_scores_schedule(wa, rows, ga, T, candidates=ids, budget_bytes=e.need_scores(1, len(rows), T, T) - 1)


# ------------------------------------------------------------------ 4. observed_at
@pytest.mark.parametrize("name", NAMES)
def test_observed_at_is_the_diagonal_of_separate_runs(name, dev):
    import torch
    from gnode.dmp import source_scores_schedule
    e, T, D = Entries(name, dev), 5, 9
    ids = list(cand_list(_n(name)))
    rows = coded_rows(name, range(2))
    wa, ga = schedules(name, PHASE)
    got = source_scores_schedule(wa, rows, ga, T, observed_at=D, candidates=ids)
    assert got.dtype == torch.float64 and got.shape == (2, len(ids), T)
    padded = np.concatenate([PHASE[:D + 1], np.full(T - 1, PHASE[D])])
    for tau in range(T):                                            # c started tau steps before D: a shift-0 call under the row from D - tau on
        wa_tau, ga_tau = schedules(name, moved(padded, D - tau, T))
        alone = source_scores_schedule(wa_tau, rows, ga_tau, T, candidates=ids)
        assert torch.equal(alone[:, :, tau], got[:, :, tau]), tau
    chunked = source_scores_schedule(wa, rows, ga, T, observed_at=D, candidates=ids, budget_bytes=e.need_scores(7, 2, T, D + T))
    assert torch.equal(chunked, got)                                # chunks of 7 samples cut through a candidate's taus
    whole = source_scores_schedule(wa, rows, ga, T, observed_at=L - 1, candidates=ids)   # the whole calendar: phase_of_step(L)
    assert whole.shape == got.shape and bool(torch.isfinite(whole).all())


# ------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("name", ["karate", "general"])
def test_refusals_leave_the_outputs_untouched(name, dev):
    import torch
    e, T, R = Entries(name, dev), 4, 2
    ids, shifts = samples(name, T)
    C = len(ids)
    cand, rows = e.up(ids, np.int32), e.up(coded_rows(name, range(R)), np.int8)
    need, need_s = e.need_scores(C, R, T), e.need_sizes(C, T)
    assert need > 0 and need_s > 0 and e.need_scores(C, R, T, T - 1) == 0 and e.need_sizes(C, T, T - 1) == 0 and e.need_scores(0, R, T) == 0
    ws = torch.empty(max(need, need_s), dtype=torch.uint8, device=dev)
    scores = torch.full((R, C, T), SENTINEL, dtype=torch.float64, device=dev)
    sizes = torch.full((C, T, 3), SENTINEL, dtype=torch.float64, device=dev)
    bad_phase = PHASE.copy(); bad_phase[L - 1] = 3                  # an entry that no sample of this call reads: still refused
    neg_phase = PHASE.copy(); neg_phase[2] = -1
    nan_w, big_g = e.up(tables(name)[0]), e.up(tables(name)[1])
    nan_w[1, 5] = float("nan"); big_g[2, 0] = 1.5
    schedule_changes = [dict(P=0), dict(P=2), dict(rows_L=T - 1), dict(phase=PHASE[:T - 1]), dict(phase=bad_phase), dict(phase=neg_phase), dict(phase=None),
                        dict(shifts=[0, 1, -1, 1, 0, 0, 0]), dict(shifts=[0, 1, L - T + 1, 1, 0, 0, 0]), dict(W=nan_w), dict(G=big_g)]
    good = dict(cand=cand, shifts=shifts, C=C, rows=rows, R=R, T=T, scores=scores, stride=C * T, ws=ws, nbytes=need)
    for change in schedule_changes + [dict(R=0), dict(C=0), dict(T=1), dict(floor=0.0), dict(stride=C * T - 1), dict(rows=None), dict(cand=None),
                                      dict(scores=None), dict(ws=None)]:
        assert e.call_scores(**dict(good, **change)) == ARG, change
    assert e.call_scores(**dict(good, W=nan_w)) == ARG and "phase 1" in e.lib.gnode_last_error().decode()      # the phase and the position are named
    assert e.call_scores(**dict(good, nbytes=need - 1)) == WORKSPACE
    good_s = dict(cand=cand, shifts=shifts, C=C, action=0, value=None, T=T, sizes=sizes, ws=ws, nbytes=need_s)
    for change in schedule_changes + [dict(C=0), dict(T=1), dict(action=2), dict(init=None), dict(cand=None), dict(sizes=None), dict(ws=None)]:
        assert e.call_sizes(**dict(good_s, **change)) == ARG, change
    assert e.call_sizes(**dict(good_s, nbytes=need_s - 1)) == WORKSPACE
    torch.cuda.synchronize()
    assert bool((scores == SENTINEL).all()) and bool((sizes == SENTINEL).all())
    assert e.call_scores(**good) == 0 and e.call_sizes(**good_s) == 0, e.lib.gnode_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(scores).all()) and bool(torch.isfinite(sizes).all())
    assert torch.equal(scores, e.scores(ids, shifts, coded_rows(name, range(R)), T)) and torch.equal(sizes, e.sizes(ids, shifts, T, "seed", False))


# ------------------------------------------------------------------ 6. end to end
def test_the_sanity_case_is_the_models(dev):
    """tests/dmp_sweep_schedule_model.py's snapshot of the tree under a three-phase lockdown: the device's scores meet the bar
    against the CPU model's float32 composition, under the schedule (observed_at = 13) and under phase 0's rates held constant,
    and its two rankings are the model's: the true source first under the schedule, and not first under constant rates."""
    import scipy.sparse as sp
    from gnode.dmp import rank_sources, source_rank_of, source_scores_events, source_scores_schedule
    from gnode.ode_nn import rate_schedule
    s = M.SANITY
    n, rp, ci, W, G, phase, snapshot = M.sanity_case()
    cands, scheduled, constant = M.sanity_tables()
    mats = [sp.csr_matrix((np.asarray(w, dtype=np.float64), ci, rp), shape=(n, n)) for w in W]
    got = source_scores_schedule(rate_schedule(mats, steps=phase), snapshot, rate_schedule(list(G), steps=phase), s["T"], observed_at=s["D"],
                                 candidates=cands)
    got_constant = source_scores_events(mats[0], snapshot, G[0], s["T"], candidates=cands)
    assert_meets_the_bar(got.cpu().numpy(), scheduled[None], [n], "sanity, scheduled")
    assert_meets_the_bar(got_constant.cpu().numpy(), constant[None], [n], "sanity, constant")
    ranked, ranked_constant = rank_sources(got[0], cands), rank_sources(got_constant[0], cands)
    assert [k for k, _, _ in ranked] == M.ranking(scheduled, cands)[0] and ranked[0][0] == s["source"] and ranked[0][1] == s["TAU"]
    assert [k for k, _, _ in ranked_constant] == M.ranking(constant, cands)[0] and ranked_constant[0][0] != s["source"]
    assert int(source_rank_of(got, cands, [s["source"]])[0]) == 0 and int(source_rank_of(got_constant, cands, [s["source"]])[0]) > 0
