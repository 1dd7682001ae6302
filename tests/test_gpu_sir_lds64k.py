"""GPU: the Monte-Carlo SIR instances that launch with MORE THAN 64 KiB of dynamic LDS, the limit gn_sir_set_attributes lifts.

Two graphs (tests/test_sir_plan.py pins their plans: "lds64k" in its GRAPHS):
  * n = 33 000: with edge_scan=True the scan keeps its state in LDS, 2 n = 66 000 B; the frontier walk (lists in the workspace,
    20 576 B of LDS) is the cross-check;
  * n = 153 000 without rows longer than 512: the frontier walk takes 65 600 B; the scan with its state in memory is the
    cross-check, and the workspace is 1.9 GB.
On each, all twelve (rate form x output x start) instances run on the large-LDS path and are compared bit for bit with the other
path; one call per graph is held to a CPU statement of the model (tests/sir_model.py, the C oracle's sir_philox)."""
import numpy as np
import pytest

from sir_cases import LDS64K_FRONTIER as FRONTIER, LDS64K_RNG as RNG, LDS64K_SCAN as SCAN_STATE, LDS64K_SIMS as SIMS, LDS64K_T as T  # noqa: F401
from sir_cases import dev, expected, graph, lds64k_case, u32  # noqa: F401

pytestmark = pytest.mark.gpu


def _case(kind, n, m):
    """graph, start and rates of a shape: (rowptr, col, DeviceGraph, seeds, p, beta, w, gamma)"""
    rp, ci, *rest = lds64k_case(kind, n, m)
    return (rp, ci, graph(kind, n, m)[2], *rest)


def _twelve(g, seeds, p, beta, w, gamma, edge_scan):
    """{(rates, output, start): tuple of numpy arrays} of the twelve instances"""
    import torch
    from gnode.ode_nn import edge_rates, initial_state, sir_counts, sir_trajectories
    out = {}
    for rname, b, gm in (("scalar", 0.45, 0.15), ("per-node", beta, gamma), ("per-edge", edge_rates(g, w), gamma)):
        for sname, start in (("seeds", seeds), ("drawn", initial_state(p))):
            out[(rname, "counts", sname)] = (u32(sir_counts(g, start, b, gm, SIMS, T, rng_seed=RNG, sim_offset=3, edge_scan=edge_scan)),)
            acc = torch.zeros((3, T, g.n), dtype=torch.int32, device="cuda")
            tr = sir_trajectories(g, start, b, gm, SIMS, T, rng_seed=RNG, sim_offset=3, counts=acc, edge_scan=edge_scan)
            out[(rname, "events", sname)] = (u32(acc), tr.t_inf.cpu().numpy(), tr.t_rec.cpu().numpy(), tr.curves.cpu().numpy())
    return out


@pytest.mark.parametrize("kind,n,m,large_is_scan", [SCAN_STATE, FRONTIER], ids=[SCAN_STATE[0], FRONTIER[0]])
def test_twelve_instances_equal_the_other_path(kind, n, m, large_is_scan, dev):
    rp, ci, g, seeds, p, beta, w, gamma = _case(kind, n, m)
    assert int(np.diff(rp).max()) <= 512                                # no long rows: the LDS figures of the docstring hold
    large = _twelve(g, seeds, p, beta, w, gamma, edge_scan=large_is_scan)
    other = _twelve(g, seeds, p, beta, w, gamma, edge_scan=not large_is_scan)
    assert len(large) == 12
    for key, arrays in large.items():
        assert arrays[0][1, 1:].any(), key
        for a, b in zip(arrays, other[key]):
            assert a.dtype == b.dtype and np.array_equal(a, b), f"{kind}: {key}"


def test_scan_with_lds_state_equals_cpu_model(dev):
    """drawn start, per-edge rates, per-node gamma, with events: counts, events, and curves rebuilt from the events"""
    import torch
    from gnode.ode_nn import edge_rates, initial_state, sir_trajectories
    kind, n, m, _ = SCAN_STATE
    rp, ci, g, seeds, p, beta, w, gamma = _case(kind, n, m)
    e = expected("init/lds64k")
    want, t_inf, t_rec = e.counts, e.t_inf, e.t_rec
    moved = int((want[0, -1] < want[0, 0]).sum())
    print(f"{kind}: the model's S row fell on {moved} nodes")
    assert moved > 100
    acc = torch.zeros((3, T, n), dtype=torch.int32, device=dev)
    tr = sir_trajectories(g, initial_state(p), edge_rates(g, w), gamma, SIMS, T, rng_seed=RNG, sim_offset=3, counts=acc, edge_scan=True)
    assert np.array_equal(u32(acc), want)
    assert np.array_equal(tr.t_inf.cpu().numpy(), t_inf) and np.array_equal(tr.t_rec.cpu().numpy(), t_rec)
    assert np.array_equal(tr.curves.cpu().numpy(), e.curves)


def test_frontier_past_64k_equals_c_oracle(dev):
    """the seed-list scalar call against the C oracle's sir_philox"""
    import oracle_c as OC
    from gnode import _lib
    from gnode.ode_nn import sir_counts
    kind, n, m, _ = FRONTIER
    rp, ci, g, seeds, *_ = _case(kind, n, m)
    assert _lib.load().gnode_sir_workspace_bytes(g.handle, T) > 1024 * 3 * 4 * n          # the 1 024 sets of global lists: 1.9 GB
    want = OC.sir_philox(n, rp, ci, seeds, 0.45, 0.15, SIMS, T, RNG, 3)
    moved = int((want[0, -1] < SIMS * want[0, 0]).sum())                                 # (row 0 holds the start once)
    print(f"{kind}: the oracle's S row fell on {moved} nodes")
    assert moved > 100
    assert np.array_equal(u32(sir_counts(g, seeds, 0.45, 0.15, SIMS, T, rng_seed=RNG, sim_offset=3)), want)
