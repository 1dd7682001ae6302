"""GPU: the DMP and mean-field comparison baselines (csrc/gnode_dmp.hip, csrc/gnode_meanfield.hip) at the graphs,
horizons, seeds and rates their goldens and the two ER cases of test_gpu_parity.py never reach.

DMP.  Through gnode.dmp.DMP_SIR, per-edge weights that are not symmetric in value, per-node gamma.  Every case is held
(a) to the float32 oracle O.dmp_sir at test_gpu_parity.py's 1e-5 relative, and
(b) to O.dmp_sir(dtype="float64"), the same recurrence in double precision.  The bar of (b) comes from the oracle, not
    from the kernel:  yard = err(float32 oracle, float64 oracle)  is what float32 costs this recurrence in numpy's
    operation order, and the kernel has to meet  gpu_err <= max(4 * yard, 1e-6)  (4: room for a different but equally
    valid rounding of the same operations; 1e-6: a floor of a few float32 ulp of 1 where yard is tiny or 0).
    Every case keeps yard <= 2.5e-5, so the bar never exceeds 1e-4.
Errors are max |a - b| / max |b| over the whole [T, n, 3] output.  Measured (yard on the CPU, gpu_err on an MI355X; the
kernel's output equalled the float32 oracle bit for bit in every case, so gpu_err = yard):

    case            yard        gpu_err
    hub             2.225e-07   2.225e-07
    isolated        3.168e-08   3.168e-08
    T2              2.980e-08   2.980e-08
    T3              3.197e-08   3.197e-08
    nnz0            3.100e-08   3.100e-08
    seeds_none      1.423e-07   1.423e-07
    seeds_all       6.842e-08   6.842e-08
    w_one           2.986e-08   2.986e-08
    w_zero          1.506e-07   1.506e-07
    gamma_01        1.153e-07   1.153e-07

w = 1 runs three steps only.  With w = 1 a node next to a seed gets phi = 1 on its outgoing edges at step 1, so
theta_2 = fl32(1 + 1e-10) - 1 = 0 exactly on them, and the cavity quotient P / theta of step 2 is 0 / 0: from output
row 3 on the reference's float32 recurrence is NaN (the float32 oracle shows the same; in float64 theta_2 = 2e-10 and
everything stays finite).  That is the model's arithmetic, which the kernel restates, not a kernel fault; rows 0..2 are
the finite part and include the P / theta quotient over theta = 1e-10 at step 1.

Mean-field.  Through gnode.ode_nn.runge_kutta_order4 (scalar gamma) or the C entry gnode_meanfield_f64 (per-node
gamma, repeated output times, the step count), against O.meanfield_rk(rtol = atol = 1e-11) at the project's 1e-6
absolute, with |S + I + R - 1| <= 1e-9.  Measured max |difference| on an MI355X: hub 1.342e-11 (56 steps), per-node
gamma 8.063e-12, repeated times 1.285e-11, isolated nodes 9.797e-12, beta = 0 against the closed form 4.957e-12.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from baseline_cases import DMP_CASES, MF_ATOL, RTOL, dmp_model as _dmp_model, dmp_parent, is_parents, er as _er, gammas as _gammas, rel as _rel, weights as _weights
from sir_cases import dev  # noqa: F401

pytestmark = pytest.mark.gpu

YARD_MAX = 2.5e-5
MF_GIVE_UP = 2000000            # gnode_meanfield_f64's step bound


def _oracle(c, dtype):
    import gnode_oracle as O
    with np.errstate(all="ignore"):     # w = 1: the float32 recurrence divides 0 by 0 in its last edge pass (module docstring)
        return O.dmp_sir(c["rp"], c["ci"], c["w"], c["gam"], c["seeds"], c["T"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def dmp_refs(name):
    """(case, float32 oracle, float64 oracle, yard), computed once; nothing here touches the GPU."""
    c = DMP_CASES[name]()
    o32, o64 = _oracle(c, "float32"), _oracle(c, "float64")
    for o in (o32, o64):
        o.setflags(write=False)
    return c, o32, o64, _rel(o32, o64)


def _dmp_gpu(c, seeds=None, T=None):
    return _dmp_model(c).run(c["seeds"] if seeds is None else seeds, c["T"] if T is None else T).cpu().numpy()


def _check_dmp(name):
    c, o32, o64, yard = dmp_refs(name)
    out = _dmp_gpu(c)
    assert out.shape == o32.shape and out.dtype == np.float32
    gpu_err = _rel(out, o64)
    print(f"dmp {name}: gpu_err={gpu_err:.3e} yard={yard:.3e} vs_fp32_oracle={_rel(out, o32):.3e}")
    assert _rel(out, o32) <= RTOL                                   # (a)
    assert yard <= YARD_MAX
    assert gpu_err <= max(4 * yard, 1e-6)                           # (b)
    assert np.max(np.abs(out.astype(np.float64).sum(-1) - 1.0)) <= 1e-5          # Ps + Pi + Pr = 1 (dmp.py:129)
    return c, out, o32


def test_dmp_hub_rows(dev):
    c, _, _ = _check_dmp("hub")
    assert np.diff(c["rp"]).max() > 500                             # a serial fp32 product of > 500 theta per node pass


def test_dmp_isolated_nodes(dev):
    c, out, o32 = _check_dmp("isolated")
    deg = np.diff(c["rp"])
    iso = np.flatnonzero(deg == 0)
    assert len(iso) > 400 and deg[c["seeds"][0]] == 0 and deg[c["seeds"][1]] > 0
    seed = np.zeros(513, np.float32); seed[c["seeds"]] = 1
    assert np.array_equal(out[:, iso, 0], np.broadcast_to(1 - seed[iso], (c["T"], len(iso))))    # empty product: Ps = Ps0
    assert np.array_equal(out[:, iso, :], o32[:, iso, :])           # no neighbour, no product: the oracle's bits
    s = c["seeds"][0]                                               # the isolated seed: Pi_t = (1 - gamma)^t
    want = (1.0 - np.float64(c["gam"][s])) ** np.arange(c["T"])
    assert np.max(np.abs(out[:, s, 1] - want)) <= 1e-6


@pytest.mark.parametrize("name", ["T2", "T3"])
def test_dmp_minimum_horizon_and_both_theta_buffers(name, dev):
    """maxTime = 2 is one node pass on theta[0]; maxTime = 3 adds one on theta[1]."""
    c, out, _ = _check_dmp(name)
    assert out.shape[0] == c["T"]


def test_dmp_graph_without_edges(dev):
    c, out, _ = _check_dmp("nnz0")
    seed = np.zeros(5, np.float32); seed[c["seeds"]] = 1
    assert np.array_equal(out[:, :, 0], np.broadcast_to(1 - seed, (c["T"], 5)))


def test_dmp_seed_lists(dev):
    c, out, _ = _check_dmp("seeds_none")
    assert np.array_equal(out, np.broadcast_to(np.array([1, 0, 0], np.float32), out.shape))     # nobody infected, exactly
    _check_dmp("seeds_all")
    assert np.array_equal(_dmp_gpu(c, seeds=[3, 77, 3]), _dmp_gpu(c, seeds=[3, 77]))            # a duplicate is one seed


@pytest.mark.parametrize("name", ["w_one", "w_zero", "gamma_01"])
def test_dmp_boundary_weights_and_rates(name, dev):
    c, out, _ = _check_dmp(name)
    assert np.isfinite(out).all()
    assert out.min() >= -1e-6 and out.max() <= 1 + 1e-6
    if name == "w_one":
        u, v = c["seeds"]
        assert v in c["ci"][c["rp"][u]:c["rp"][u + 1]]              # the two seeds are adjacent
        nb = c["ci"][c["rp"][u]:c["rp"][u + 1]]
        nb = nb[nb != v]
        assert len(nb) and np.all(out[1, nb, 0] <= 1e-9)            # certain transmission: Ps = theta = 1e-10 after one step
    if name == "w_zero":
        assert (c["w"] == 0).sum() == -(-len(c["w"]) // 3)
    if name == "gamma_01":
        assert c["gam"][0] == 0 and c["gam"][1] == 1
        assert not out[:, 0, 2].any()                               # gamma = 0: never recovered
        assert out[1, 1, 2] == 1 and out[1, 1, 1] == 0              # gamma = 1: recovered after one step


@pytest.mark.parametrize("name", list(DMP_CASES))
def test_dmp_seed_entry_is_the_parents_bits(name, dev):
    """tests/golden/dmp_parent.json: the output of gnode_dmp_f32 at commit 893d874 on an MI355X, by digest and with no
    tolerance, and the workspace that the seed entry and the initial-state entry asked for there."""
    from gnode import _lib
    c = DMP_CASES[name]()
    m = _dmp_model(c)
    assert is_parents(f"dmp_f32/{name}", m.run(c["seeds"], c["T"]))
    lib, want = _lib.load(), dmp_parent()[f"dmp_f32/{name}"]["workspace_bytes"]
    assert lib.gnode_dmp_workspace_bytes(m.graph.handle) == want and lib.gnode_dmp_init_workspace_bytes(m.graph.handle) == want


def test_dmp_workspace_carries_nothing_between_runs(dev):
    c, _, _, _ = dmp_refs("seeds_none")
    m = _dmp_model(c)
    a = m.run([3, 77], 8).cpu().numpy()
    b = m.run([200], 5).cpu().numpy()
    again = m.run([3, 77], 8).cpu().numpy()
    assert np.array_equal(a, _dmp_gpu(c, seeds=[3, 77], T=8))
    assert np.array_equal(b, _dmp_gpu(c, seeds=[200], T=5))
    assert np.array_equal(again, a)


def test_dmp_bad_arguments_raise_and_the_handle_survives(dev):
    import torch
    from gnode import _lib
    from gnode._lib import GnodeError
    c, _, _, _ = dmp_refs("seeds_none")
    n = len(c["rp"]) - 1
    m = _dmp_model(c)
    good = m.run([3, 77], 8).cpu().numpy()
    for seeds, T in (([3, 77], 1), ([3, n], 8), ([-1, 3], 8)):
        with pytest.raises(GnodeError):
            m.run(seeds, T)
        assert np.array_equal(m.run([3, 77], 8).cpu().numpy(), good)
    # a workspace one byte short, through the C entry
    lib = _lib.load()
    need = lib.gnode_dmp_workspace_bytes(m.graph.handle)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty((8, n, 3), dtype=torch.float32, device=dev)
    seeds = np.array([3, 77], np.int32)
    call = lambda nbytes: lib.gnode_dmp_f32(m.graph.handle, _lib.ptr(m.weights), _lib.ptr(m.nodes_gamma), _lib.host_ptr(seeds), 2, 8,
                                            _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_ptr())
    with pytest.raises(GnodeError):
        _lib.check(call(need - 1))
    _lib.check(call(need))
    assert np.array_equal(out.cpu().numpy(), good)


def test_dmp_refuses_one_missing_reverse_edge_in_a_large_pattern(dev):
    """A 1 000-node symmetric pattern with one directed entry taken out of the middle of the CSR: refused, whichever of
    the graph handle and the DMP setup pass finds it; a symmetric pattern is served afterwards."""
    import scipy.sparse as sp
    from gnode.dmp import DMP_SIR
    from gnode._lib import GnodeError
    rp, ci, _ = _er(1000, 4000, 9)
    k = len(ci) // 2                                                # deep inside: neither the first nor the last row
    row = int(np.searchsorted(rp, k, side="right") - 1)
    assert 100 < row < 900
    rp2 = rp.copy(); rp2[row + 1:] -= 1
    ci2 = np.delete(ci, k)
    w = _weights(len(ci), 0.05, 0.4, 19)
    gam = _gammas(1000, 20)
    with pytest.raises(GnodeError):
        DMP_SIR(sp.csr_matrix((np.delete(w, k), ci2, rp2), shape=(1000, 1000)), gam).run([1, 500], 5)
    import gnode_oracle as O
    out = DMP_SIR(sp.csr_matrix((w, ci, rp), shape=(1000, 1000)), gam).run([1, 500], 5).cpu().numpy()
    assert _rel(out, O.dmp_sir(rp, ci, w, gam, [1, 500], 5)) <= RTOL


# ------------------------------------------------------------------ mean-field
def _meanfield_entry(dev, rp, ci, seeds, beta, gamma, t_out, rtol=1e-10, atol=1e-12, ws_short=0):
    """gnode_meanfield_f64 as it stands (runge_kutta_order4's defaults): (I, S, R) float64 [len(t_out), n] and the step count."""
    import torch
    from gnode import _lib
    from gnode.graph import DeviceGraph
    lib = _lib.load()
    g = DeviceGraph(rp, ci)
    n = g.n
    seeds = np.ascontiguousarray(seeds, dtype=np.int32)
    t_out = np.ascontiguousarray(t_out, dtype=np.float64)
    gam = torch.from_numpy(np.array(np.broadcast_to(np.asarray(gamma, np.float64), (n,)))).to(dev)      # a writable copy
    out = torch.empty((3, len(t_out), n), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.gnode_meanfield_workspace_bytes(g.handle), dtype=torch.uint8, device=dev)
    steps = C.c_int64(-1)
    _lib.check(lib.gnode_meanfield_f64(g.handle, _lib.host_ptr(seeds), int(seeds.shape[0]), float(beta), _lib.ptr(gam),
                                       _lib.host_ptr(t_out), int(len(t_out)), float(rtol), float(atol), _lib.ptr(out[0]),
                                       _lib.ptr(out[1]), _lib.ptr(out[2]), C.byref(steps), _lib.ptr(ws), ws.numel() - ws_short,
                                       _lib.stream_ptr()))
    o = out.cpu().numpy()
    return o[0], o[1], o[2], int(steps.value)


def _meanfield_wrapper(rp, ci, seeds, beta, gamma, maxTime):
    import scipy.sparse as sp
    from gnode import ode_nn
    n = len(rp) - 1
    A = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
    return ode_nn.runge_kutta_order4(ode_nn.sir, A, n, seeds, beta, gamma, 1, maxTime)


def _mf_reference(rp, ci, seeds, beta, gamma, maxTime):
    import gnode_oracle as O
    return O.meanfield_rk(rp, ci, seeds, beta, gamma, 1, maxTime, rtol=1e-11, atol=1e-11)


def _check_mf(tag, got, want):
    diff = max(float(np.max(np.abs(g - w))) for g, w in zip(got, want))
    print(f"meanfield {tag}: max |gpu - reference| = {diff:.3e}")
    for g, w in zip(got, want):
        assert g.shape == w.shape
    assert diff <= MF_ATOL
    assert np.max(np.abs(got[0] + got[1] + got[2] - 1.0)) <= 1e-9
    return diff


def test_meanfield_hub_graph(dev):
    import gnode_oracle as O
    rp, ci, _ = O.chung_lu_graph(2001, 25000, seed=2)
    assert np.diff(rp).max() > 500
    got = _meanfield_wrapper(rp, ci, [3, 1500], 0.002, 0.2, 8)
    want = _mf_reference(rp, ci, [3, 1500], 0.002, 0.2, 8)
    _check_mf("hub", got, want)
    I, S, R, steps = _meanfield_entry(dev, rp, ci, [3, 1500], 0.002, 0.2, np.arange(8.0))
    assert all(np.array_equal(a, b) for a, b in zip((I, S, R), got))          # the wrapper is this call
    print(f"meanfield hub: {steps} steps")
    assert 0 < steps < MF_GIVE_UP
    others = np.setdiff1d(np.arange(2001), [3, 1500])                         # the case is not trivial: in the REFERENCE the
    assert (want[0][-1, others] > 100 * MF_ATOL).sum() > 1000                 # infection reaches most nodes far above the bar


def test_meanfield_per_node_gamma(dev):
    rp, ci, _ = _er(700, 3000, 11)
    gam = np.random.default_rng(21).uniform(0.05, 0.6, size=700)
    I, S, R, steps = _meanfield_entry(dev, rp, ci, [0, 350], 0.05, gam, np.arange(10.0))
    _check_mf("per-node gamma", (I, S, R), _mf_reference(rp, ci, [0, 350], 0.05, gam, 10))
    assert 0 < steps < MF_GIVE_UP
    flat = _mf_reference(rp, ci, [0, 350], 0.05, float(gam.mean()), 10)       # the per-node rates matter at this bar
    assert max(np.max(np.abs(a - b)) for a, b in zip((I, S, R), flat)) > 100 * MF_ATOL


def test_meanfield_without_seeds_keeps_the_initial_state(dev):
    """Nobody infected: every stage derivative is 0, the error norm is exactly 0 (the controller's e == 0 branch grows the
    step fivefold) and every output row is the initial state to the bit."""
    rp, ci, _ = _er(700, 3000, 11)
    I, S, R = _meanfield_wrapper(rp, ci, [], 0.05, 0.2, 9)
    assert I.shape == (9, 700)
    assert np.array_equal(S, np.ones_like(S)) and not I.any() and not R.any()
    _, _, _, steps = _meanfield_entry(dev, rp, ci, [], 0.05, 0.2, np.arange(9.0))
    assert 8 <= steps <= 8 + 6                   # h = 1e-3 * 5^k reaches the unit spacing within 5 steps of the first interval


def test_meanfield_beta_zero_is_pure_recovery(dev):
    rp, ci, _ = _er(700, 3000, 11)
    gamma, seeds, T = 0.3, [0, 350], 8
    I, S, R = _meanfield_wrapper(rp, ci, seeds, 0.0, gamma, T)
    seed = np.zeros(700); seed[seeds] = 1.0
    assert np.array_equal(S, np.broadcast_to(1.0 - seed, S.shape))            # dS = -0 * (A I) S: exactly constant
    decay = np.exp(-gamma * np.arange(T))[:, None] * seed[None, :]
    diff = max(np.max(np.abs(I - decay)), np.max(np.abs(R - (seed[None, :] - decay))))
    print(f"meanfield beta=0: max |gpu - closed form| = {diff:.3e}")
    assert diff <= 1e-7
    assert np.max(np.abs(I + S + R - 1.0)) <= 1e-9


def test_meanfield_repeated_output_times(dev):
    rp, ci, _ = _er(700, 3000, 11)
    I, S, R, steps = _meanfield_entry(dev, rp, ci, [0, 350], 0.05, 0.2, [0.0, 1.0, 1.0, 2.0])
    for a in (I, S, R):
        assert a.shape == (4, 700) and np.array_equal(a[1], a[2])             # bitwise: no step is taken between them
    want = _mf_reference(rp, ci, [0, 350], 0.05, 0.2, 3)
    _check_mf("repeated times", tuple(a[[0, 1, 3]] for a in (I, S, R)), want)
    assert 0 < steps < MF_GIVE_UP


def test_meanfield_isolated_nodes_and_ragged_n(dev):
    rp, ci, _ = _er(257, 30, 12)                                    # 257 = 256 + 1: a second workgroup with one live thread
    deg = np.diff(rp)
    iso, con = int(np.flatnonzero(deg == 0)[-1]), int(np.flatnonzero(deg > 0)[0])
    assert (deg == 0).sum() > 150 and deg[256] == 0 and iso == 256
    gamma, T = 0.25, 8
    got = _meanfield_wrapper(rp, ci, [iso, con], 0.4, gamma, T)
    _check_mf("isolated", got, _mf_reference(rp, ci, [iso, con], 0.4, gamma, T))
    I, S, R = got
    others = np.setdiff1d(np.flatnonzero(deg == 0), [iso])
    assert np.array_equal(S[:, others], np.ones((T, len(others)))) and not I[:, others].any() and not R[:, others].any()
    assert np.max(np.abs(I[:, iso] - np.exp(-gamma * np.arange(T)))) <= 1e-7  # an isolated seed only recovers
    assert I[-1, ci[rp[con]:rp[con + 1]]].max() > 0.01                        # the connected seed did infect its neighbours


def test_meanfield_bad_arguments_raise(dev):
    from gnode._lib import GnodeError
    rp, ci, _ = _er(257, 30, 12)
    ok = dict(seeds=[3], beta=0.1, gamma=0.2, t_out=[0.0, 1.0, 2.0])
    good = _meanfield_entry(dev, rp, ci, **ok)
    for bad in (dict(t_out=[0.5, 1.0, 2.0]), dict(t_out=[0.0, 2.0, 1.0]), dict(rtol=0.0), dict(seeds=[257]), dict(seeds=[3, -1]),
                dict(ws_short=1)):
        with pytest.raises(GnodeError):
            _meanfield_entry(dev, rp, ci, **{**ok, **bad})
        again = _meanfield_entry(dev, rp, ci, **ok)
        assert all(np.array_equal(a, b) for a, b in zip(again[:3], good[:3])) and again[3] == good[3]
