"""GPU: the mean-field with per-node and per-contact rates for a batch of samples (gnode_meanfield_rates_f64,
csrc/gnode_meanfield.hip) through `gnode.ode_nn.runge_kutta_order4`, `gnode.ode_nn.meanfield_batch` and the C entry.

Yardstick: tests/meanfield_rates_model.py (scipy odeint at rtol = atol = 1e-11, held to the reference's own vectors by
tests/test_meanfield_rates_model.py) at the project's mean-field bar, 1e-6 absolute on probabilities, with
|S + I + R - 1| <= 1e-9.  The bit-for-bit tests compare with gnode_meanfield_f64 / gnode_meanfield_init_f64 as they stand.
Every maximum difference is printed.  Measured on an MI355X: golden karate 1.951e-08 and er150 3.536e-08 (LSODA's own error at
its default tolerances); against the model B = 3 5.4e-11, isolated + self-loop 8.5e-11, star 2.1e-10, no edges against the
closed form 4.9e-12; batch against solo 3.2e-12 (151 shared steps, solo 138 / 152 / 143); 0 against the scalar entries."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from meanfield_rates_model import MF_ATOL, golden_case, max_diff, meanfield_rates, one_hot

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_WORKSPACE = -1, -3
SENTINEL = -7.25


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gnode import _lib
    _lib.load()                       # fails loudly if libgnode_hip.so is missing
    return torch.device("cuda:0")


# ------------------------------------------------------------------ graphs (numpy only)
def _csr(n, edges):
    """Sorted symmetric CSR of the undirected edges (a self-loop is stored once)."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    r, c = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    a = sp.coo_matrix((np.ones(len(r)), (r, c)), shape=(n, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32)


def _er(n, m, seed):
    import gnode_oracle as O
    rp, ci, _ = O.er_graph(n, m, seed=seed)
    return np.asarray(rp, np.int32), np.asarray(ci, np.int32)


def _adjacency(rp, ci):
    n = len(rp) - 1
    return sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))


# ------------------------------------------------------------------ the C entries as they stand
def _up(dev, a):
    import torch
    return None if a is None or np.size(a) == 0 else torch.from_numpy(np.array(a, dtype=np.float64)).to(dev)


def _rates_entry(dev, rp, ci, init, beta, w, gamma, t_out, graph=None, ws_short=0, rtol=1e-10, atol=1e-12):
    """gnode_meanfield_rates_f64 at runge_kutta_order4's tolerances.  init [B, n, 3], beta [B, n] or None, w [nnz] or None,
    gamma [B, n].  Returns (status, (I, S, R) float64 [B, len(t_out), n], steps); the outputs start out as SENTINEL."""
    import torch
    from gnode import _lib
    from gnode.graph import DeviceGraph
    lib = _lib.load()
    g = graph or DeviceGraph(rp, ci)
    init = np.asarray(init, dtype=np.float64)
    B, n = init.shape[0], init.shape[1]
    assert n == g.n
    t_out = np.ascontiguousarray(t_out, dtype=np.float64)
    y0, bet, wd, gam = _up(dev, init), _up(dev, beta), _up(dev, w), _up(dev, gamma)
    out = torch.full((3, len(t_out), B * n), SENTINEL, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.gnode_meanfield_rates_workspace_bytes(g.handle, B), dtype=torch.uint8, device=dev)
    steps = C.c_int64(-1)
    status = lib.gnode_meanfield_rates_f64(g.handle, B, _lib.ptr(y0), _lib.ptr(bet), _lib.ptr(wd), _lib.ptr(gam),
                                           _lib.host_ptr(t_out), int(len(t_out)), float(rtol), float(atol), _lib.ptr(out[0]),
                                           _lib.ptr(out[1]), _lib.ptr(out[2]), C.byref(steps), _lib.ptr(ws), ws.numel() - ws_short,
                                           _lib.stream_ptr())
    torch.cuda.synchronize()
    o = out.cpu().numpy().reshape(3, len(t_out), B, n).transpose(0, 2, 1, 3)
    return status, (o[0], o[1], o[2]), int(steps.value)


def _scalar_entry(dev, rp, ci, start, beta, gamma, t_out):
    """gnode_meanfield_f64 (start = a seed list) or gnode_meanfield_init_f64 (start = [n, 3]): ((I, S, R), steps)."""
    import torch
    from gnode import _lib
    from gnode.graph import DeviceGraph
    lib = _lib.load()
    g = DeviceGraph(rp, ci)
    n = g.n
    t_out = np.ascontiguousarray(t_out, dtype=np.float64)
    gam = _up(dev, np.broadcast_to(np.asarray(gamma, np.float64), (n,)))
    out = torch.empty((3, len(t_out), n), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.gnode_meanfield_workspace_bytes(g.handle), dtype=torch.uint8, device=dev)
    steps = C.c_int64(-1)
    tail = (float(beta), _lib.ptr(gam), _lib.host_ptr(t_out), int(len(t_out)), 1e-10, 1e-12, _lib.ptr(out[0]), _lib.ptr(out[1]),
            _lib.ptr(out[2]), C.byref(steps), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    if np.ndim(start) == 2:
        y0 = _up(dev, start)
        _lib.check(lib.gnode_meanfield_init_f64(g.handle, _lib.ptr(y0), *tail))
    else:
        seeds = np.ascontiguousarray(start, dtype=np.int32)
        _lib.check(lib.gnode_meanfield_f64(g.handle, _lib.host_ptr(seeds), int(seeds.shape[0]), *tail))
    o = out.cpu().numpy()
    return (o[0], o[1], o[2]), int(steps.value)


def _check(tag, got, want):
    diff = max_diff(got, want)
    print(f"meanfield rates {tag}: max |gpu - model| = {diff:.3e}")
    for g, w in zip(got, want):
        assert np.shape(g) == np.shape(w)
    assert diff <= MF_ATOL
    assert np.max(np.abs(np.asarray(got[0]) + got[1] + got[2] - 1.0)) <= 1e-9
    return diff


# ------------------------------------------------------------------ golden vectors of the reference
@pytest.mark.parametrize("name", ["karate", "er150"])
def test_golden_through_runge_kutta_order4(name, dev):
    from gnode.ode_nn import edge_rates, runge_kutta_order4, sir
    d = golden_case(name)
    rp, ci = d["rowptr"], d["col"]
    n = len(rp) - 1
    beta = edge_rates((rp, ci), d["w"]) if d["w"] is not None else d["beta"]
    gamma = d["gamma"] if name == "karate" else float(d["gamma"][0])            # er150: a number beside per-node beta
    got = runge_kutta_order4(sir, _adjacency(rp, ci), n, d["seeds"], beta, gamma, d["deltaT"], d["maxTime"])
    diff = max_diff(got, (d["I"], d["S"], d["R"]))
    print(f"meanfield rates golden {name}: max |gpu - reference| = {diff:.3e}")
    assert got[0].shape == (d["maxTime"], n)
    assert diff <= MF_ATOL
    assert np.max(np.abs(got[0] + got[1] + got[2] - 1.0)) <= 1e-9


# ------------------------------------------------------------------ bit for bit with the scalar entries
def _er150():
    d = golden_case("er150")
    return d["rowptr"], d["col"]


def _same(tag, new, steps_new, old, steps_old):
    print(f"meanfield rates {tag}: steps {steps_new} / {steps_old}, max |new - scalar entry| = {max_diff(new, old):.3e}")
    assert all(np.array_equal(a[0], b) for a, b in zip(new, old))             # a[0]: the batch's one sample
    assert steps_new == steps_old > 0


def test_b1_constant_beta_is_the_seed_entry_bit_for_bit(dev):
    rp, ci = _er150()
    n, t_out, gam = 150, np.arange(9.0), np.random.default_rng(3).uniform(0.1, 0.5, size=150)
    old, steps_old = _scalar_entry(dev, rp, ci, [3, 77], 0.05, gam, t_out)
    assert old[0][-1].max() > 1e-3
    init = one_hot(n, [3, 77])[None]
    st, new, steps = _rates_entry(dev, rp, ci, init, np.full((1, n), 0.05), None, gam[None], t_out)
    assert st == 0
    _same("w NULL", new, steps, old, steps_old)
    st, new, steps = _rates_entry(dev, rp, ci, init, np.full((1, n), 0.05), np.ones(len(ci)), gam[None], t_out)
    assert st == 0
    _same("w ones", new, steps, old, steps_old)


def test_b1_constant_beta_is_the_init_entry_bit_for_bit(dev):
    from sir_model import mixed_init
    rp, ci = _er150()
    n, t_out = 150, np.arange(9.0)
    p, _ = mixed_init(n, 5)
    old, steps_old = _scalar_entry(dev, rp, ci, p, 0.05, 0.3, t_out)
    for tag, w in (("init, w NULL", None), ("init, w ones", np.ones(len(ci)))):
        st, new, steps = _rates_entry(dev, rp, ci, p[None], np.full((1, n), 0.05), w, np.full((1, n), 0.3), t_out)
        assert st == 0
        _same(tag, new, steps, old, steps_old)


# ------------------------------------------------------------------ direction of the weights
PATH_RP, PATH_CI = np.array([0, 1, 3, 4], np.int32), np.array([1, 0, 2, 1], np.int32)


def _path_rates():
    from gnode.ode_nn import edge_rates
    M = sp.csr_matrix(([0.5, 0.5], ([0, 1], [1, 2])), shape=(3, 3))            # 0 -> 1 -> 2, nothing flows back
    er = edge_rates((PATH_RP, PATH_CI), M)
    assert er.w.tolist() == [0.5, 0.0, 0.5, 0.0]
    return er


def _check_direction(up, down):
    """up: seed {2}, the end of the chain; down: seed {0}, its start.  Each (I, S, R) [T, 3]."""
    I, S, R = up
    assert np.array_equal(S[:, :2], np.ones_like(S[:, :2])) and np.array_equal(I[:, :2], np.zeros_like(I[:, :2]))
    assert I[1, 2] < 1.0 and R[-1, 2] > 0.5                                    # the seed itself recovers
    I, S, R = down
    assert I[-1, 2] > 1e-3 and I[-1, 1] > 1e-3 and S[-1, 2] < 1.0


def test_weights_point_from_row_to_column(dev):
    from gnode.ode_nn import runge_kutta_order4, sir
    er, A = _path_rates(), _adjacency(PATH_RP, PATH_CI)
    _check_direction(runge_kutta_order4(sir, A, 3, [2], er, 0.3, 1, 10), runge_kutta_order4(sir, A, 3, [0], er, 0.3, 1, 10))


def test_weights_point_from_row_to_column_in_a_batch(dev):
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import meanfield_batch
    out = meanfield_batch(DeviceGraph(PATH_RP, PATH_CI), [[2], [0]], _path_rates(), 0.3, maxTime=10)
    assert out.I.shape == (2, 10, 3) and out.I.is_cuda
    I, S, R = (t.cpu().numpy() for t in out)
    _check_direction((I[0], S[0], R[0]), (I[1], S[1], R[1]))


# ------------------------------------------------------------------ ragged shapes
B3_T = 9


@pytest.fixture(scope="module")
def b3(dev):
    """B = 3 on n = 300: 900 rows, so samples 0 / 1 and 1 / 2 share the 256-thread blocks 1 and 2.  Seeds, beta rows and
    gamma rows differ per sample.  The batch through the C entry, once."""
    rp, ci = _er(300, 900, 7)
    rng = np.random.default_rng(17)
    c = dict(rp=rp, ci=ci, seeds=[[5], [250, 31], [299]], beta=rng.uniform(0.02, 0.2, size=(3, 300)),
             gamma=rng.uniform(0.1, 0.5, size=(3, 300)))
    init = np.stack([one_hot(300, s) for s in c["seeds"]])
    st, c["got"], c["steps"] = _rates_entry(dev, rp, ci, init, c["beta"], None, c["gamma"], np.arange(float(B3_T)))
    assert st == 0
    return c


def test_batch_of_three_against_the_model(b3):
    for b in range(3):
        want = meanfield_rates(b3["rp"], b3["ci"], one_hot(300, b3["seeds"][b]), b3["beta"][b], None, b3["gamma"][b], B3_T)
        _check(f"B=3 sample {b}", tuple(a[b] for a in b3["got"]), want)
        assert want[0][-1].max() > 1000 * MF_ATOL
    assert max_diff(tuple(a[0] for a in b3["got"]), tuple(a[2] for a in b3["got"])) > 1000 * MF_ATOL     # the samples differ


def test_meanfield_batch_is_the_entry(b3, dev):
    from gnode.graph import DeviceGraph
    from gnode.ode_nn import meanfield_batch
    out = meanfield_batch(DeviceGraph(b3["rp"], b3["ci"]), b3["seeds"], b3["beta"], b3["gamma"], maxTime=B3_T)
    assert out.S.shape == (3, B3_T, 300)
    assert all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(out, b3["got"]))


def test_batch_against_solo_runs(b3, dev):
    """One shared step size: a sample inside the batch differs from its solo run at the level of the tolerances only."""
    solo_steps = []
    for b in range(3):
        st, solo, steps = _rates_entry(dev, b3["rp"], b3["ci"], one_hot(300, b3["seeds"][b])[None], b3["beta"][b][None], None,
                                       b3["gamma"][b][None], np.arange(float(B3_T)))
        assert st == 0
        solo_steps.append(steps)
        diff = max_diff(tuple(a[b] for a in b3["got"]), tuple(a[0] for a in solo))
        print(f"meanfield rates B=3 sample {b}: max |batch - solo| = {diff:.3e}")
        assert diff <= MF_ATOL
    print(f"meanfield rates B=3: {b3['steps']} shared steps, solo {solo_steps}")


def test_isolated_node_self_loop_and_ragged_n(dev):
    """n = 257 = 256 + 1: a second workgroup with one live thread, which is the isolated node; node 5 has a self-loop, which
    is its own reverse entry and counts once."""
    from gnode.ode_nn import edge_rates, runge_kutta_order4, sir
    import gnode_oracle as O
    _, _, e = O.er_graph(257, 500, seed=12)
    e = np.asarray(e)
    e = np.concatenate([e[(e != 256).all(axis=1)], [[5, 5]]])
    rp, ci = _csr(257, e)
    assert rp[257] == rp[256] and 5 in ci[rp[5]:rp[6]]
    rng = np.random.default_rng(23)
    w, gam, T = rng.uniform(0.05, 0.4, size=len(ci)), rng.uniform(0.1, 0.5, size=257), 8
    got = runge_kutta_order4(sir, _adjacency(rp, ci), 257, [256, 5], edge_rates((rp, ci), w), gam, 1, T)
    _check("isolated + self-loop", got, meanfield_rates(rp, ci, one_hot(257, [256, 5]), None, w, gam, T))
    assert np.max(np.abs(got[0][:, 256] - np.exp(-gam[256] * np.arange(T)))) <= 1e-7     # an isolated seed only recovers
    others = np.setdiff1d(ci[rp[5]:rp[6]], [5])
    assert others.size and got[0][-1, others].min() > 0.01                     # the looped seed did infect its neighbours


def test_star_with_per_edge_weights(dev):
    """600 leaves: the hub's row is one thread's 600-entry gather, every leaf's a single entry; the seed is a leaf."""
    from gnode.ode_nn import edge_rates, runge_kutta_order4, sir
    n = 601
    rp, ci = _csr(n, [(0, v) for v in range(1, n)])
    w, T = np.random.default_rng(29).uniform(0.05, 0.6, size=len(ci)), 8
    got = runge_kutta_order4(sir, _adjacency(rp, ci), n, [7], edge_rates((rp, ci), w), 0.2, 1, T)
    want = meanfield_rates(rp, ci, one_hot(n, [7]), None, w, 0.2, T)
    _check("star", got, want)
    assert want[0][-1, 0] > 0.01 and want[0][-1, 1:].max() > 0.01 and np.ptp(want[0][-1, 8:]) > 1000 * MF_ATOL


def test_no_edges_is_pure_recovery(dev):
    n, T = 5, 8
    rp, ci = np.zeros(n + 1, np.int32), np.zeros(0, np.int32)
    gam = np.random.default_rng(31).uniform(0.1, 0.5, size=(2, n))
    seeds = [[1, 3], [0]]
    init = np.stack([one_hot(n, s) for s in seeds])
    st, (I, S, R), steps = _rates_entry(dev, rp, ci, init, None, None, gam, np.arange(float(T)))
    assert st == 0 and steps > 0
    seed = init[:, :, 1]
    assert np.array_equal(S, np.broadcast_to((1.0 - seed)[:, None, :], S.shape))         # dS = -(0 * S): exactly constant
    decay = np.exp(-gam[:, None, :] * np.arange(T)[None, :, None]) * seed[:, None, :]
    diff = max(np.max(np.abs(I - decay)), np.max(np.abs(R - (seed[:, None, :] - decay))))
    print(f"meanfield rates nnz=0: max |gpu - closed form| = {diff:.3e}")
    assert diff <= 1e-7
    assert np.max(np.abs(I + S + R - 1.0)) <= 1e-9


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_usable(dev):
    from gnode import _lib
    from gnode.graph import DeviceGraph
    lib = _lib.load()
    rp, ci = _er(257, 400, 12)
    g = DeviceGraph(rp, ci)
    rng = np.random.default_rng(37)
    init = np.stack([one_hot(257, [3]), one_hot(257, [200, 9])])
    ok = dict(init=init, beta=rng.uniform(0.05, 0.3, size=(2, 257)), w=rng.uniform(0.2, 1.0, size=len(ci)),
              gamma=rng.uniform(0.1, 0.5, size=(2, 257)), t_out=np.arange(6.0), graph=g)
    st, good, steps = _rates_entry(dev, rp, ci, **ok)
    assert st == 0 and steps > 0
    st, out, _ = _rates_entry(dev, rp, ci, **ok, ws_short=1)
    assert st == ERR_WORKSPACE and b"workspace" in lib.gnode_last_error()
    assert all(np.all(a == SENTINEL) for a in out)                             # nothing was written
    for bad in (dict(t_out=[0.5, 1.0]), dict(t_out=[0.0, 2.0, 1.0]), dict(rtol=0.0)):
        st, out, _ = _rates_entry(dev, rp, ci, **{**ok, **bad})
        assert st == ERR_ARG and all(np.all(a == SENTINEL) for a in out)
    st, again, steps_again = _rates_entry(dev, rp, ci, **ok)
    assert st == 0 and steps_again == steps and all(np.array_equal(a, b) for a, b in zip(again, good))
    _check("after the refusals", tuple(a[1] for a in again),
           meanfield_rates(rp, ci, init[1], ok["beta"][1], ok["w"], ok["gamma"][1], 6))


def test_asymmetric_pattern_with_weights_is_refused(dev):
    from gnode import _lib
    lib = _lib.load()
    rp, ci = np.array([0, 1, 3, 3], np.int32), np.array([1, 0, 2], np.int32)   # 0 <-> 1, 1 -> 2 without its reverse entry
    init, gam, t_out = one_hot(3, [0])[None], np.full((1, 3), 0.3), np.arange(4.0)
    st, out, _ = _rates_entry(dev, rp, ci, init, None, np.full(3, 0.5), gam, t_out)
    assert st == ERR_ARG and b"symmetric" in lib.gnode_last_error()
    assert all(np.all(a == SENTINEL) for a in out)
    st, out, _ = _rates_entry(dev, rp, ci, init, None, None, gam, t_out)       # w NULL builds no table: row 1 reads 0 and 2
    assert st == 0 and out[0][0, -1, 1] > 1e-3 and np.array_equal(out[1][0, :, 2], np.ones(4))
