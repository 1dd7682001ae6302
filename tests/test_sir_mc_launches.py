"""No GPU: what the five calls of the Monte-Carlo candidate sweep hand to the library -- the groups, the records packed per
group, the slices of the accumulators and the order of the arguments -- recorded with the library, the pointers and the graph
handle replaced by stubs, on the CPU.  Every expected value is written out from the rule the docstrings and include/gnode.h
state: arguments 0 .. 10 are (handle, init, candidates, shifts, C, action, phase, P, L, W, G); then the group's evidence and the
call's scalars; then (sims, sim_offset, T, seed); then the outputs; then (workspace, its bytes, stream, edge_scan)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from sir_host_cases import N, RING, _obs

HANDLE, OWN_HANDLE, STREAM, WS_BYTES = 0x1234, 0x5678, 0x9ABC, 4096
CAND, SIMS = [0, 3, -1], 10
C_ = len(CAND)
SHARED = dict(graph=RING, beta=0.3, gamma=0.2, sims=SIMS, candidates=CAND, device="cpu")


class Library:
    """Every attribute is a function that records (name, args); a size query answers WS_BYTES, an entry 0."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        def fn(*args):
            self.log.append((name, args))
            return WS_BYTES if name.endswith("workspace_bytes") else 0
        return fn


@pytest.fixture
def rec(monkeypatch):
    from gnode import _lib, ode_nn
    lib = Library()
    lib.graphs = []

    def device_graph(rowptr, col):
        lib.graphs.append((rowptr, col))
        return SimpleNamespace(handle=HANDLE)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "ptr", lambda t: t)
    monkeypatch.setattr(_lib, "host_ptr", lambda a: a)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: STREAM)
    monkeypatch.setattr(_lib, "check", lambda status: None)
    monkeypatch.setattr(ode_nn, "DeviceGraph", device_graph)
    return lib


def _split(log, query, entry):
    """(the size queries' argument lists, the launches' argument lists) of a log that holds them in turn, a query before its launch"""
    assert [name for name, _ in log] == [query, entry] * (len(log) // 2) and len(log) % 2 == 0
    return [a for _, a in log[0::2]], [a for _, a in log[1::2]]


def _view(part, whole, o0, og):
    """`part` is rows o0 .. o0 + og - 1 of the contiguous `whole`, in its memory"""
    per = int(np.prod(whole.shape[1:]))
    assert tuple(part.shape) == (og, *whole.shape[1:]) and part.dtype == whole.dtype and part.is_contiguous()
    assert part.untyped_storage().data_ptr() == whole.untyped_storage().data_ptr() and part.storage_offset() == whole.storage_offset() + o0 * per


def _head(args, T, handle=HANDLE, action=0):
    """arguments 0 .. 10 for the ring under constant rates, nobody infected at the start, no shifts"""
    assert args[0] == handle
    assert args[1].dtype == np.float64 and np.array_equal(args[1], np.tile([1.0, 0.0, 0.0], (N, 1)))
    assert args[2].dtype == np.int32 and args[2].tolist() == CAND
    assert args[3].dtype == np.int32 and args[3].tolist() == [0] * C_
    assert args[4:6] == (C_, action)
    assert args[6].dtype == np.int32 and args[6].tolist() == [0] * T           # constants are one phase, L = T calendar steps
    assert args[7:9] == (1, T)
    assert np.array_equal(args[9], np.full((1, 2 * N), 0.3)) and np.array_equal(args[10], np.full((1, N), 0.2))
    return args[:11]


def _tail(args, at, T, seed=None, sim_offset=0, edge_scan=0, outputs=1):
    """(sims, sim_offset, T, seed) at `at`, then `outputs` outputs, then the last four; returns the seed"""
    assert args[at:at + 3] == (SIMS, sim_offset, T) and len(args) == at + 4 + outputs + 4
    ws = args[-4]
    assert ws.dtype.is_floating_point is False and ws.element_size() == 1 and ws.numel() == WS_BYTES and args[-3:] == (WS_BYTES, STREAM, edge_scan)
    assert type(args[-1]) is int
    if seed is not None:
        assert args[at + 3].value == seed
    return args[at + 3].value


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert isinstance(y, np.ndarray) and x.dtype == y.dtype and np.array_equal(x, y)
        elif hasattr(x, "value"):
            assert x.value == y.value
        else:
            assert type(x) is type(y) and x == y


SNAP = [0, 1, 2, -1, 0, 0]
# seven evidence sets of 1, 2, 3, 1, 4, 2, 3 records: (rows, offsets), and the records by row and then by node as (node, offset, kind)
SETS = [
    ([[-1, 3, -1, -1, -1, -1]], [0]),
    ([[0, -1, -1, -1, -1, 1]], [-2]),
    ([[-1, -1, 2, -1, -1, -1], [4, -1, 2, -1, -1, -1]], [-3, 0]),
    ([[-1, -1, -1, -1, 0, -1]], [-1]),
    ([[-1, 1, -1, -1, 3, -1], [2, -1, -1, -1, 1, -1]], [-1, 0]),
    ([[-1, -1, -1, 1, -1, -1], [-1, -1, -1, 2, -1, -1]], [-4, -2]),
    ([[1, 1, -1, -1, -1, 0]], [-5]),
]
RECORDS = [
    [(1, 0, 3)],
    [(0, -2, 0), (5, -2, 1)],
    [(2, -3, 2), (0, 0, 4), (2, 0, 2)],
    [(4, -1, 0)],
    [(1, -1, 1), (4, -1, 3), (0, 0, 2), (4, 0, 1)],
    [(3, -4, 1), (3, -2, 2)],
    [(0, -5, 1), (1, -5, 1), (5, -5, 0)],
]


def _evidence(count):
    return [_obs(*SETS[i % len(SETS)]) for i in range(count)]


def _packed(args, first, count):
    """arguments 11 .. 16 of a launch on the evidence sets first .. first + count - 1: which, node, off, kind, R, og"""
    recs = [RECORDS[i % len(RECORDS)] for i in range(first, first + count)]
    which, node, off, kind = args[11:15]
    assert all(a.dtype == np.int32 and a.flags["C_CONTIGUOUS"] for a in (which, node, off, kind))
    assert which.tolist() == [i for i, r in enumerate(recs) for _ in r]      # a set is named by its place in the group
    assert list(zip(node.tolist(), off.tolist(), kind.tolist())) == [x for r in recs for x in r]
    R = sum(len(r) for r in recs)
    assert args[15:17] == (R, count)
    return R


# -------------------------------------------------------------------------------------------------------------- snapshots
def test_source_scores_mc_sends_17_snapshots_as_16_and_1(rec):
    from gnode.ode_nn import source_scores_mc
    T, bins = 4, 5
    obs = np.asarray([SNAP[o % N:] + SNAP[:o % N] for o in range(17)], np.int8)
    out = source_scores_mc(obs=obs, maxTime=T, measure="match", bins=bins, rng_seed=-1, edge_scan=True, **SHARED)
    assert tuple(out.hist.shape) == (17, C_, T, bins + 1) and out.hist.dtype.is_floating_point is False and out.hist.element_size() == 8
    assert (out.sims, out.bins, out.squeezed) == (SIMS, bins, False) and len(rec.graphs) == 1
    queries, launches = _split(rec.log, "gnode_sir_sweep_scores_workspace_bytes", "gnode_sir_mc_philox_sweep_scores")
    assert queries == [(HANDLE, T, 1, T, C_, 16), (HANDLE, T, 1, T, C_, 1)]
    for args, (o0, og) in zip(launches, ((0, 16), (16, 1))):
        _head(args, T)
        assert args[11].dtype == np.int8 and np.array_equal(args[11], obs[o0:o0 + og]) and args[12:15] == (og, 1, bins)      # "match" is 1
        _tail(args, 15, T, seed=2**64 - 1, edge_scan=1)
        _view(args[19], out.hist, o0, og)
    assert launches[1][19].storage_offset() == 16 * C_ * T * (bins + 1)
    rec.log.clear()
    one = source_scores_mc(obs=SNAP, maxTime=T, **SHARED)            # the defaults: jaccard is 0, 64 bins, no edge scan
    (query,), (args,) = _split(rec.log, "gnode_sir_sweep_scores_workspace_bytes", "gnode_sir_mc_philox_sweep_scores")
    assert query == (HANDLE, T, 1, T, C_, 1) and args[12:15] == (1, 0, 64) and one.squeezed and args[19] is not None
    assert _tail(args, 15, T) < 2**62
    _view(args[19], one.hist, 0, 1)


# ---------------------------------------------------------------------------------------------------------- timed records
def test_source_scores_timed_mc_groups_by_the_cells_and_packs_the_records(rec):
    from gnode.ode_nn import source_scores_timed_mc
    T = 300                                                         # min(16, 2048 // 300) = 6 sets per launch
    out = source_scores_timed_mc(observations=_evidence(7), maxTime=T, sim_offset=3, **SHARED)
    bins = 4                                                        # the largest record count
    assert tuple(out.hist.shape) == (7, C_, T, bins + 1) and (out.sims, out.bins, out.squeezed) == (SIMS, bins, False)
    queries, launches = _split(rec.log, "gnode_sir_sweep_timed_workspace_bytes", "gnode_sir_mc_philox_sweep_timed")
    assert len(launches) == 2
    seeds = []
    for query, args, (o0, og) in zip(queries, launches, ((0, 6), (6, 1))):
        _head(args, T)
        R = _packed(args, o0, og)
        assert R == (13, 3)[o0 > 0] and query == (HANDLE, T, 1, T, C_, og, R) and args[17] == bins
        seeds.append(_tail(args, 18, T, sim_offset=3))
        _view(args[22], out.hist, o0, og)
    assert seeds[0] == seeds[1] < 2**62                            # drawn once for the call
    assert launches[1][22].storage_offset() == 6 * C_ * T * (bins + 1)


# -------------------------------------------------------------------------------------------------------------- posteriors
def test_the_two_posteriors_send_17_sets_as_16_and_1_and_differ_by_mismatches(rec):
    import torch
    from gnode.ode_nn import posterior_states_mc, posterior_strata_mc
    T, now, hz, M = 4, 1, [0, 2], 1
    H, D = len(hz), M + 1
    kw = dict(observations=_evidence(17), maxTime=T, now=now, horizons=hz, rng_seed=77, **SHARED)
    post = posterior_states_mc(**kw)
    log, rec.log = rec.log, []
    given = torch.zeros((17, C_, D), dtype=torch.int64)
    strata = posterior_strata_mc(accepted=given, **kw)                # mismatches = 1 by default
    assert tuple(post.counts.shape) == (17, H, 2, N) and tuple(post.accepted.shape) == (17, C_)
    assert tuple(strata.counts.shape) == (17, D, H, 2, N) and strata.accepted is given
    assert (post.sims, post.now, post.horizons, post.squeezed) == (SIMS, now, (0, 2), False) == (strata.sims, strata.now, strata.horizons, strata.squeezed)
    assert strata.records == tuple(len(RECORDS[i % 7]) for i in range(17))
    q_post, l_post = _split(log, "gnode_sir_sweep_posterior_workspace_bytes", "gnode_sir_mc_philox_sweep_posterior")
    q_strata, l_strata = _split(rec.log, "gnode_sir_sweep_posterior_workspace_bytes", "gnode_sir_mc_philox_sweep_posterior_strata")
    assert q_post == q_strata and len(l_post) == len(l_strata) == 2  # the strata have no size query of their own
    for query, a, b, (o0, og) in zip(q_post, l_post, l_strata, ((0, 16), (16, 1))):
        _head(a, T)
        R = _packed(a, o0, og)
        assert query == (HANDLE, T, 1, T, C_, og, R, H)
        assert a[17] == now and a[18].dtype == np.int32 and a[18].tolist() == hz and a[19] == H and b[20] == M and type(b[20]) is int
        _tail(a, 20, T, seed=77, outputs=2)
        _tail(b, 21, T, seed=77, outputs=2)
        _same(a[:20], b[:20])
        _same(a[20:24], b[21:25])
        assert a[27:] == b[28:]
        _view(a[24], post.counts, o0, og)
        _view(a[25], post.accepted, o0, og)
        _view(b[25], strata.counts, o0, og)
        _view(b[26], given, o0, og)
    assert (l_post[1][24].storage_offset(), l_post[1][25].storage_offset()) == (16 * H * 2 * N, 16 * C_)
    assert (l_strata[1][25].storage_offset(), l_strata[1][26].storage_offset()) == (16 * D * H * 2 * N, 16 * C_ * D)


# ---------------------------------------------------------------------------------------------------------- outbreak sizes
def test_outbreak_sizes_mc_makes_one_query_and_one_launch(rec):
    import torch
    from gnode.ode_nn import outbreak_sizes_mc
    T = 4
    sums = torch.zeros((C_, T, 3), dtype=torch.int64)
    out = outbreak_sizes_mc(maxTime=T, start=[1], action="immunise", sums=sums, **SHARED)
    assert out.sums is sums and out.ever is None and out.sims == SIMS
    (query,), (args,) = _split(rec.log, "gnode_sir_sweep_workspace_bytes", "gnode_sir_mc_philox_sweep")
    assert query == (HANDLE, T, 1, T, C_) and args[0] == HANDLE and args[5] == 1       # "immunise" is 1
    assert np.array_equal(args[1], np.asarray([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]] + [[1.0, 0.0, 0.0]] * 4))
    _tail(args, 11, T, outputs=2)
    assert args[15] is sums and args[16] is None
    rec.log.clear()
    out = outbreak_sizes_mc(maxTime=T, per_trajectory=True, **SHARED)
    (query,), (args,) = _split(rec.log, "gnode_sir_sweep_workspace_bytes", "gnode_sir_mc_philox_sweep")
    _head(args, T)
    _tail(args, 11, T, outputs=2)
    assert args[15] is out.sums and tuple(out.sums.shape) == (C_, T, 3) and out.sums.dtype == torch.int64 and not out.sums.any()
    assert args[16] is out.ever and tuple(out.ever.shape) == (C_, SIMS) and out.ever.dtype == torch.int32


# ---------------------------------------------------------------------------------------------------------- all five calls
def _five(T=4, **more):
    """(name of the entry, where sims stands, outputs, the call) for the five calls on equal shared inputs"""
    from gnode.ode_nn import outbreak_sizes_mc, posterior_states_mc, posterior_strata_mc, source_scores_mc, source_scores_timed_mc
    kw = dict(SHARED, maxTime=T, **more)
    ev = _evidence(2)
    return [
        ("gnode_sir_mc_philox_sweep", 11, 2, lambda **k: outbreak_sizes_mc(**dict(kw, **k))),
        ("gnode_sir_mc_philox_sweep_scores", 15, 1, lambda **k: source_scores_mc(obs=[SNAP, SNAP], **dict(kw, **k))),
        ("gnode_sir_mc_philox_sweep_timed", 18, 1, lambda **k: source_scores_timed_mc(observations=ev, **dict(kw, **k))),
        ("gnode_sir_mc_philox_sweep_posterior", 20, 2, lambda **k: posterior_states_mc(observations=ev, now=1, horizons=(0, 2), **dict(kw, **k))),
        ("gnode_sir_mc_philox_sweep_posterior_strata", 21, 2, lambda **k: posterior_strata_mc(observations=ev, now=1, horizons=(0, 2), mismatches=2, **dict(kw, **k))),
    ]


def test_the_five_calls_share_the_head_and_the_tail_of_the_arguments(rec):
    T = 4
    heads = []
    for entry, at, outputs, call in _five(T):
        rec.log.clear()
        call(rng_seed=-1, sim_offset=5, edge_scan=1.0)              # (anything true is 1)
        (name, args), = [x for x in rec.log if not x[0].endswith("workspace_bytes")]
        assert name == entry and isinstance(args[at + 3], ctypes.c_uint64)
        heads.append(_head(args, T))
        _tail(args, at, T, seed=2**64 - 1, sim_offset=5, edge_scan=1, outputs=outputs)
    for head in heads[1:]:
        _same(head, heads[0])
    assert len(rec.graphs) == 5 and all(np.array_equal(rp, RING[0]) and np.array_equal(ci, RING[1]) for rp, ci in rec.graphs)


def test_no_trajectories_make_the_handle_and_call_nothing(rec):
    import torch
    zeros = []
    for _, _, _, call in _five(sims=0):
        before = len(rec.graphs)
        out = call()
        assert len(rec.graphs) == before + 1 and rec.log == [] and out.sims == 0
        zeros.append([tuple(t.shape) for t in out[:2] if isinstance(t, torch.Tensor)])
        assert all(t.dtype == torch.int64 and not t.any() for t in out[:2] if isinstance(t, torch.Tensor))
    assert zeros == [[(C_, 4, 3)], [(2, C_, 4, 65)], [(2, C_, 4, 3)], [(2, 2, 2, N), (2, C_)], [(2, 3, 2, 2, N), (2, C_, 3)]]
    out = _five(sims=0)[0][3](per_trajectory=True)
    assert tuple(out.ever.shape) == (C_, 0) and out.ever.dtype == torch.int32 and rec.log == []


def test_a_given_accumulator_is_returned_and_sliced(rec):
    import torch
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64)      # noqa: E731
    five = _five()
    for (entry, at, outputs, call), given in zip(five, (dict(sums=i64(C_, 4, 3)), dict(hist=i64(2, C_, 4, 65)), dict(hist=i64(2, C_, 4, 3)),
                                                        dict(counts=i64(2, 2, 2, N), accepted=i64(2, C_)),
                                                        dict(counts=i64(2, 3, 2, 2, N), accepted=i64(2, C_, 3)))):
        rec.log.clear()
        out = call(**given)
        args = rec.log[-1][1]
        for j, (name, t) in enumerate(given.items()):
            assert getattr(out, name) is t
            if name == "sums":
                assert args[at + 4] is t
            else:
                _view(args[at + 4 + j], t, 0, 2)


def test_a_graph_that_has_a_handle_is_used_as_it_is(rec):
    own = SimpleNamespace(handle=OWN_HANDLE, n=N, nnz=2 * N, rowptr=RING[0], col=RING[1])
    for entry, at, outputs, call in _five():
        rec.log.clear()
        call(graph=own)
        assert [args[0] for _, args in rec.log] == [OWN_HANDLE, OWN_HANDLE] and rec.log[-1][0] == entry
    assert rec.graphs == []
