"""GPU: DMP with rates that change over time (gnode_dmp_batch_schedule_f32 through gnode.dmp.dmp_batch and through the C
entry) on the cases of tests/baseline_cases.py: B = 3 mixed states, three phases with different weights and gammas.  A
schedule that changes nothing returns dmp_batch's BITS; a sample of a batch is its B = 1 scheduled run bit for bit; against
tests/dmp_schedule_model.py the bars are those of test_gpu_dmp_batch.py::test_batch_meets_the_models_bars; and on the tree
20 000 scheduled Monte-Carlo trajectories lie within the project's 5-sigma bound of the scheduled DMP and far outside it of
the constant one."""
import functools

import numpy as np
import pytest

import schedule_cases as K
from baseline_cases import DMP_CASES, RTOL, assert_schedule_parents, gammas as _gammas, rel as _rel, schedule_entry, weights as _weights
from dmp_schedule_model import dmp_sir_schedule
from sir_cases import dev, dmp_ratio, er_of as _er_of, state as _state, u32 as _u32  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = ["w_zero", "T3", "hub", "T2", "nnz0"]
CASE_SEED = {name: 1700 + 10 * i for i, name in enumerate(CASES)}
SCALE = [1.0, 0.5, 0.8125]
LDS_WORKGROUP = 160 * 1024
PATTERN = [0, 0, 0, 0, 1, 1, 2, 2, 0, 0, 1, 2]            # phases revisited, a change at the last step of T = 12 and T = 10
ARG, WORKSPACE = -1, -3                                    # GNODE_ERR_ARG, GNODE_ERR_WORKSPACE of include/gnode.h


def _phase(T):
    return np.asarray({2: [0, 1], 3: [0, 2, 1]}.get(T, PATTERN[:T]), dtype=np.int32)


def _matrix(rp, ci, w):
    import scipy.sparse as sp
    n = len(rp) - 1
    return sp.csr_matrix((np.asarray(w, dtype=np.float64), ci, rp), shape=(n, n))


@functools.lru_cache(maxsize=None)
def sched_case(name):
    """(case, phase [T], W three float32 [nnz] tables, G three float32 tables -- [3, n] per sample, [n], [n] --, B = 3 states);
    read-only, numpy only"""
    from sir_model import mixed_init
    c = DMP_CASES[name]()
    n, nnz, seed = len(c["rp"]) - 1, len(c["ci"]), CASE_SEED[name]
    W = [c["w"], (c["w"] * np.float32(0.5)).astype(np.float32), _weights(nnz, 0.02, 0.3, seed + 1)]
    if nnz:
        W[2][::4] = 0.0
    G = [np.stack([c["gam"], (c["gam"] * np.float32(0.5)).astype(np.float32), _gammas(n, seed + 2)]), _gammas(n, seed + 3),
         (c["gam"] * np.float32(1.5)).astype(np.float32)]
    ps = [mixed_init(n, seed + 5 + b)[0] for b in range(3)]
    for a in W + G + ps:
        a.setflags(write=False)
    return c, _phase(c["T"]), W, G, ps


def _sample_tables(name, b):
    """sample b's per-phase tables, as the call forms them: float32(float64(data_p) * scale[b]) and its gamma"""
    c, phase, W, G, ps = sched_case(name)
    return [(W[p].astype(np.float64) * SCALE[b]).astype(np.float32) for p in range(3)], [G[0][b], G[1], G[2]]


@functools.lru_cache(maxsize=None)
def sched_out(name):
    """the scheduled batch through dmp_batch, once: a float32 host tensor [3, T, n, 3]"""
    from gnode.dmp import dmp_batch
    from gnode.ode_nn import rate_schedule
    c, phase, W, G, ps = sched_case(name)
    return dmp_batch(rate_schedule([_matrix(c["rp"], c["ci"], w) for w in W], steps=phase), [_state(p) for p in ps],
                     rate_schedule(list(G), steps=phase), c["T"], scale=rate_schedule([SCALE], starts=[1])).cpu()


def _handle_of(c):
    from gnode.graph import DeviceGraph
    return DeviceGraph(c["rp"], c["ci"])


def test_which_form_serves_which_case(dev):
    from gnode import _lib
    lib = _lib.load()
    size = {}
    for name in ("w_zero", "T3", "hub"):
        g = _handle_of(DMP_CASES[name]())
        size[name] = int(lib.gnode_dmp_batch_lds_bytes(g.handle))
    assert 0 < size["w_zero"] <= LDS_WORKGROUP and 0 < size["T3"] <= LDS_WORKGROUP < size["hub"]


@pytest.mark.parametrize("name", CASES)
def test_a_schedule_that_changes_nothing_returns_dmp_batchs_bits(name, dev):
    import torch
    from gnode.dmp import dmp_batch
    from gnode.ode_nn import rate_schedule
    c, phase, W, G, ps = sched_case(name)
    M, starts, T = _matrix(c["rp"], c["ci"], W[0]), [_state(p) for p in ps], c["T"]
    want = dmp_batch(M, starts, G[0], T, scale=SCALE)
    assert torch.isfinite(want).all()
    one = dmp_batch(rate_schedule([M], starts=[1]), starts, rate_schedule([G[0]], starts=[1]), T, scale=rate_schedule([SCALE], starts=[1]))
    assert torch.equal(one, want)
    same = dmp_batch(rate_schedule([M, M, M], steps=phase), starts, rate_schedule([G[0]] * 3, steps=phase), T,
                     scale=rate_schedule([SCALE, SCALE], steps=np.arange(T) % 2))
    assert torch.equal(same, want)
    shared = dmp_batch(M, starts, rate_schedule([G[1], G[1]], steps=np.arange(T) % 2), T)      # shared tables: strides 0
    assert torch.equal(shared, dmp_batch(M, starts, G[1], T))


@pytest.mark.parametrize("name", CASES)
def test_scheduled_batch_meets_the_models_bars(name, dev):
    c, phase, W, G, ps = sched_case(name)
    out = sched_out(name).numpy()
    assert out.shape == (3, c["T"], len(c["rp"]) - 1, 3)
    for b in range(3):
        Wb, Gb = _sample_tables(name, b)
        o32, o64 = (dmp_sir_schedule(c["rp"], c["ci"], Wb, Gb, phase, ps[b], c["T"], d) for d in ("float32", "float64"))
        yard, gpu_err = _rel(o32, o64), _rel(out[b], o64)
        print(f"dmp schedule {name}[{b}]: gpu_err={gpu_err:.3e} yard={yard:.3e} vs_fp32_restatement={_rel(out[b], o32):.3e}")
        assert _rel(out[b], o32) <= RTOL
        assert gpu_err <= max(4 * yard, 1e-6)
        assert np.max(np.abs(out[b].astype(np.float64).sum(-1) - 1.0)) <= 1e-5
        assert np.array_equal(out[b][0], ps[b].astype(np.float32))             # row 0 is the start
    if len(c["ci"]) and c["T"] > 2:                                 # the schedule matters: the constant run differs
        const = dmp_sir_schedule(c["rp"], c["ci"], [_sample_tables(name, 0)[0][0]], [G[0][0]], np.zeros(c["T"], int), ps[0], c["T"])
        assert _rel(out[0], const) > 100 * RTOL


def test_schedules_with_different_change_points(dev):
    """weight_adj, scale and gamma schedules that change at different steps: the joint phases, against the model per step"""
    from gnode.dmp import dmp_batch
    from gnode.ode_nn import rate_schedule
    c, _, W, G, ps = sched_case("w_zero")
    T, rp, ci = c["T"], c["rp"], c["ci"]
    wa = rate_schedule([_matrix(rp, ci, W[0]), _matrix(rp, ci, W[2])], starts=[1, 6])
    sc = rate_schedule([None, SCALE, 0.75], steps=[0, 0, 1, 1, 2, 2, 0, 0, 1, 1, 2, 2])
    gm = rate_schedule([G[0], 0.3, G[2]], starts=[1, 3, 9])
    out = dmp_batch(wa, [_state(p) for p in ps], gm, T, scale=sc).cpu().numpy()
    pw, psc, pg = (s.phase_of_step(T) for s in (wa, sc, gm))
    for b in range(3):
        data, s_of = [W[0], W[2]], [1.0, SCALE[b], 0.75]
        Wt = [np.zeros(len(ci), np.float32)] + [(data[pw[t]].astype(np.float64) * s_of[psc[t]]).astype(np.float32) for t in range(1, T)]
        Gt = [np.zeros(34, np.float32)] + [[G[0][b], np.full(34, 0.3, np.float32), G[2]][pg[t]] for t in range(1, T)]
        o32 = dmp_sir_schedule(rp, ci, Wt, Gt, np.arange(T), ps[b], T, "float32")
        assert _rel(out[b], o32) <= RTOL, b


# ------------------------------------------------------------------------------------------------------------ the C entry
class Entry:
    """gnode_dmp_batch_schedule_f32 on one graph with device tensors of the caller's making."""

    def __init__(self, c, dev):
        from gnode import _lib
        self.lib, self.dev, self.g = _lib.load(), dev, _handle_of(c)

    def need(self, B, T):
        return int(self.lib.gnode_dmp_batch_schedule_workspace_bytes(self.g.handle, B, T))

    def up(self, a, dtype=np.float32):
        import torch
        a = np.ascontiguousarray(a, dtype=dtype)
        return None if a.size == 0 else torch.from_numpy(a).to(self.dev)

    def call(self, w, w_stride, gam, gamma_stride, phase, P, init, B, T, out, ws, nbytes=None):
        from gnode import _lib
        ph = None if phase is None else _lib.host_ptr(phase)
        return self.lib.gnode_dmp_batch_schedule_f32(self.g.handle, _lib.ptr(w), w_stride, _lib.ptr(gam), gamma_stride, ph, P, _lib.ptr(init), B, T,
                                                     _lib.ptr(out), _lib.ptr(ws), ws.numel() if nbytes is None else nbytes, _lib.stream_ptr())


@pytest.mark.parametrize("name", ["w_zero", "hub"])
def test_a_sample_of_a_batch_is_its_own_run_with_shared_and_per_sample_strides(name, dev):
    import torch
    c, phase, W, G, ps = sched_case(name)
    n, nnz, B, T, P = len(c["rp"]) - 1, len(c["ci"]), 3, c["T"], 3
    e = Entry(c, dev)
    assert (e.lib.gnode_dmp_batch_lds_bytes(e.g.handle) <= LDS_WORKGROUP) == (name == "w_zero")
    Wb = np.stack([np.stack(_sample_tables(name, b)[0]) for b in range(B)])                 # [B][P][nnz]
    Gb = np.stack([np.stack(_sample_tables(name, b)[1]) for b in range(B)])                 # [B][P][n]
    init = e.up(np.stack(ps))
    ws, ws1 = (torch.empty(e.need(b, T), dtype=torch.uint8, device=dev) for b in (B, 1))
    for w_shared in (True, False):                                  # (w_stride, gamma_stride) = (0, P n) and (P nnz, 0)
        w, gam = (Wb[0], Gb) if w_shared else (Wb, Gb[0])
        out = torch.zeros((B, T, n, 3), dtype=torch.float32, device=dev)
        assert e.call(e.up(w), 0 if w_shared else P * nnz, e.up(gam), P * n if w_shared else 0, phase, P, init, B, T, out, ws) == 0, \
            e.lib.gnode_last_error().decode()
        for b in range(B):
            solo = torch.zeros((1, T, n, 3), dtype=torch.float32, device=dev)
            assert e.call(e.up(Wb[0 if w_shared else b]), 0, e.up(Gb[b if w_shared else 0]), 0, phase, P, init[b:b + 1], 1, T, solo, ws1) == 0
            assert torch.isfinite(solo).all() and torch.equal(out[b], solo[0]), f"{name}, shared weights {w_shared}: sample {b}"
    assert torch.equal(out.cpu()[0], sched_out(name)[0])            # the last call's sample 0 has the tables of dmp_batch's sample 0


@pytest.mark.parametrize("name", ["T3", "hub"])
def test_refusals_leave_out_untouched_and_a_good_call_is_served(name, dev):
    import torch
    c, phase, W, G, ps = sched_case(name)
    n, nnz, B, T, P = len(c["rp"]) - 1, len(c["ci"]), 2, c["T"], 3
    e = Entry(c, dev)
    Wp, Gp = np.stack(_sample_tables(name, 0)[0]), np.stack(_sample_tables(name, 0)[1])
    w, gam, init = e.up(Wp), e.up(Gp), e.up(np.stack(ps[:B]))
    need = e.need(B, T)
    assert e.need(0, T) == 0 and e.need(B, 1) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.full((B, T, n, 3), -7.0, dtype=torch.float32, device=dev)
    assert e.call(w, 0, gam, 0, phase, P, init, B, T, out, ws, need - 1) == WORKSPACE
    assert e.call(w, 0, gam, 0, phase, P, init, 0, T, out, ws) == ARG
    assert e.call(w, 0, gam, 0, phase, P, init, B, 1, out, ws) == ARG
    assert e.call(w, 0, gam, 0, phase, 0, init, B, T, out, ws) == ARG
    assert e.call(w, 0, gam, 0, phase, 2, init, B, T, out, ws) == ARG and "phase[" in e.lib.gnode_last_error().decode()      # a phase of 2 with P = 2
    bad = phase.copy(); bad[T - 1] = -1
    assert e.call(w, 0, gam, 0, bad, P, init, B, T, out, ws) == ARG
    for ws_, gs_ in ((nnz, 0), (P * nnz - 1, 0), (0, n), (0, P * n + 1), (-P * nnz, 0), (1, 0)):
        assert e.call(w, ws_, gam, gs_, phase, P, init, B, T, out, ws) == ARG, (ws_, gs_)
    for missing in ("w", "gam", "init", "out", "ws", "phase"):
        a = dict(w=w, gam=gam, init=init, out=out, ws=ws, phase=phase)
        a[missing] = None
        from gnode import _lib
        assert e.lib.gnode_dmp_batch_schedule_f32(e.g.handle, _lib.ptr(a["w"]), 0, _lib.ptr(a["gam"]), 0,
                                                  None if a["phase"] is None else _lib.host_ptr(a["phase"]), P, _lib.ptr(a["init"]), B, T,
                                                  _lib.ptr(a["out"]), _lib.ptr(a["ws"]), need, _lib.stream_ptr()) == ARG, missing
    said = lambda: e.lib.gnode_last_error().decode()                # noqa: E731
    for bad in (float("nan"), 1.5, -0.25):                          # a rate that is no probability: phase and position named
        if nnz:
            x = Wp.copy(); x[2, nnz - 1] = bad
            assert e.call(e.up(x), 0, gam, 0, phase, P, init, B, T, out, ws) == ARG and "phase 2" in said() and f"weights[{nnz - 1}]" in said()
        x = np.stack([Gp, Gp]); x[1, 1, 3] = bad                    # per-sample tables: the sample is named too
        assert e.call(w, 0, e.up(x), P * n, phase, P, init, B, T, out, ws) == ARG
        assert "sample 1" in said() and "phase 1" in said() and "gamma[3]" in said()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    free = phase.copy(); free[0] = 99                               # entry 0 is never read
    assert e.call(w, 0, gam, 0, free, P, init, B, T, out, ws) == 0, e.lib.gnode_last_error().decode()
    for b in range(B):
        o32 = dmp_sir_schedule(c["rp"], c["ci"], list(Wp), list(Gp), phase, ps[b], T, "float32")
        assert _rel(out[b].cpu().numpy(), o32) <= RTOL


# ------------------------------------------------------------------------------------------------------- the parent's bits
PARENT_CASES = [(name, "per_sample") for name in CASES] + [(name, "shared") for name in ("w_zero", "hub")]


def parent_entries(name, tables, dev):
    """[(key, entry)] of tests/golden/dmp_schedule_parent.json for one case: `sched_out` (per-sample weights and phase-0 gammas,
    three phases), or one matrix and two different gamma tables alternating, shared by the samples (both strides 0)."""
    from gnode import _lib
    from gnode.dmp import dmp_batch
    from gnode.ode_nn import rate_schedule
    c, phase, W, G, ps = sched_case(name)
    T, lib, g = c["T"], _lib.load(), _handle_of(c)
    if tables == "per_sample":
        out = sched_out(name)
    else:
        out = dmp_batch(_matrix(c["rp"], c["ci"], W[0]), [_state(p) for p in ps], rate_schedule([G[1], G[2]], steps=np.arange(T) % 2), T)
    return [(f"forward/{name}/{tables}", schedule_entry([out], lib.gnode_dmp_batch_schedule_workspace_bytes(g.handle, 3, T),
                                                        lib.gnode_dmp_batch_lds_bytes(g.handle) <= LDS_WORKGROUP))]


@pytest.mark.parametrize("name,tables", PARENT_CASES)
def test_outputs_are_the_parents_bits(name, tables, dev):
    """tests/golden/dmp_schedule_parent.json: what the library of commit 8bd479b returned on an MI355X, when the scheduled
    marginals had kernels and a host side of their own."""
    assert_schedule_parents(parent_entries(name, tables, dev))


# --------------------------------------------------------------------------------------------------------------- the tree
def test_monte_carlo_meets_the_scheduled_dmp_on_the_tree_and_not_the_constant_one(dev):
    import torch
    from gnode.dmp import dmp_batch
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import rate_schedule, sir_counts
    import sir_model as M
    n, rp, ci, W, G, p = K.tree()
    g = DeviceGraph(rp, ci)
    counts = sir_counts(g, _state(p), rate_schedule([_er_of(g, w) for w in W], steps=K.TREE_PHASE), rate_schedule(list(G), steps=K.TREE_PHASE),
                        K.TREE_SIMS, K.TREE_T, K.TREE_RNG, device=dev)
    cnt = _u32(counts)
    assert np.array_equal(cnt, M.counts(*K.tree_events(), K.TREE_T, hold_row0=False))
    mats = [_matrix(rp, ci, w) for w in W]
    for m in mats[1:]:                                              # one pattern: the zeros of a phase are stored
        assert np.array_equal(m.indices, mats[0].indices) and m.nnz == len(ci)
    P_sched = dmp_batch(rate_schedule(mats, steps=K.TREE_PHASE), [_state(p)], rate_schedule(list(G), steps=K.TREE_PHASE), K.TREE_T)[0]
    P_const = dmp_batch(mats[0], [_state(p)], G[0], K.TREE_T)[0]
    assert torch.isfinite(P_sched).all()
    right = dmp_ratio(cnt, K.TREE_SIMS, P_sched.cpu().numpy().astype(np.float64))
    const = dmp_ratio(cnt, K.TREE_SIMS, P_const.cpu().numpy().astype(np.float64))
    print(f"tree: sigma ratio against the scheduled DMP {right:.2f}, against constant rates {const:.1f}")
    assert right <= 5.0
    assert const > 5.0
