"""GPU: Monte-Carlo SIR labels with per-node infection and recovery rates (gnode_sir_mc_philox_nodes through sir_counts /
sir_torch).  Every comparison is np.array_equal on uint32 counts: against the scalar call where the arrays are constant
(the coins do not move), against the CPU model of tests/sir_model.py on the cases of tests/sir_cases.py (held to the oracle
by tests/test_sir_model.py) where they are not."""
import numpy as np
import pytest

from sir_cases import IDS, SHAPES, bfs_depth, case, dev, expected, graph, live_nodes, node_rates, u32  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,n,m,seeds,sims,T", SHAPES, ids=IDS)
def test_constant_arrays_equal_scalar_call(kind, n, m, seeds, sims, T, dev):
    """The feature's main invariant: arrays that hold one constant each return the scalar call's counts, bit for bit --
    both arrays, array beta with scalar gamma, and the reverse; numpy, list and torch (GPU) inputs."""
    import torch
    from gnode.ode_nn import sir_counts
    rp, ci, g = graph(kind, n, m)
    for beta, gamma, rs in ((0.45, 0.15, 11), (0.05, 0.6, 12)):
        want = u32(sir_counts(g, seeds, beta, gamma, sims, T, rng_seed=rs, sim_offset=5))
        assert want[1, 1:].any()
        forms = (("both", np.full(n, beta), np.full(n, gamma)), ("beta", [beta] * n, gamma),
                 ("gamma", beta, torch.full((n,), gamma, dtype=torch.float64, device=dev)))
        for what, b, gm in forms:
            got = u32(sir_counts(g, seeds, b, gm, sims, T, rng_seed=rs, sim_offset=5))
            assert np.array_equal(got, want), f"{kind}: per-node call with constant {what} != scalar call (beta={beta})"
        got = u32(sir_counts(g, seeds, np.full(n, beta), np.full(n, gamma), sims, T, rng_seed=rs, sim_offset=5, edge_scan=True))
        assert np.array_equal(got, want), f"{kind}: per-node edge scan with constant arrays != scalar call (beta={beta})"


@pytest.mark.parametrize("kind,n,m,seeds,sims,T", SHAPES, ids=IDS)
def test_heterogeneous_rates_equal_cpu_model(kind, n, m, seeds, sims, T, dev):
    """Frontier walk and edge scan with a different beta and gamma on every node, shielded (beta = 0), certain
    (beta = 1), never-recovering and always-recovering nodes among them, against the CPU model.  The model's output is
    first checked for a live epidemic, so that two dead ones cannot pass for agreement."""
    from gnode.ode_nn import sir_counts
    g = graph(kind, n, m)[2]
    c, want = case(f"nodes/{kind}"), expected(f"nodes/{kind}").counts
    seeds, beta, gamma = c.start, c.beta, c.gamma
    live_nodes(c, expected(f"nodes/{kind}"))
    a = u32(sir_counts(g, seeds, beta, gamma, sims, T, rng_seed=21))
    assert np.array_equal(a, want), f"{kind}: frontier walk != CPU model"
    b = u32(sir_counts(g, seeds, beta, gamma, sims, T, rng_seed=21, edge_scan=True))
    assert np.array_equal(b, want), f"{kind}: edge scan != CPU model"


def test_large_state_paths(dev):
    """n = 100 000: the scan kernel keeps the trajectory state in memory, the frontier walk its lists (int32 ids)."""
    from gnode.ode_nn import sir_counts
    c, want = case("nodes/large"), expected("nodes/large").counts
    g, seeds, beta, gamma = graph("large", c.n, c.m)[2], c.start, c.beta, c.gamma
    assert (want[0, -1] < 24).sum() > 1000
    assert np.array_equal(u32(sir_counts(g, seeds, beta, gamma, 24, 8, rng_seed=99)), want)
    assert np.array_equal(u32(sir_counts(g, seeds, beta, gamma, 24, 8, rng_seed=99, edge_scan=True)), want)


def test_more_than_32_seeds(dev):
    """40 seeds: the list is copied from the host instead of travelling as a kernel argument."""
    from gnode.ode_nn import sir_counts
    c, want = case("nodes/seeds40"), expected("nodes/seeds40").counts
    g, seeds, beta, gamma = graph("er-small", c.n, c.m)[2], c.start, c.beta, c.gamma
    assert len(seeds) == 40 and max(seeds) < c.n
    assert np.array_equal(u32(sir_counts(g, seeds, beta, gamma, 50, 8, rng_seed=31)), want)
    assert np.array_equal(u32(sir_counts(g, seeds, beta, gamma, 50, 8, rng_seed=31, edge_scan=True)), want)


def test_sharded_equals_whole(dev):
    """Two shards of the sims range accumulated into one array equal one call, with heterogeneous rates."""
    import torch
    from gnode.ode_nn import sir_counts
    n, seeds = 500, [3, 499]
    rp, ci, g = graph("er-small", n, 2500)
    beta, gamma, _ = node_rates("er-small", n, seeds)
    whole = sir_counts(g, seeds, beta, gamma, 1000, 12, rng_seed=5)
    acc = sir_counts(g, seeds, beta, gamma, 600, 12, rng_seed=5, sim_offset=0)
    acc = sir_counts(g, seeds, beta, gamma, 400, 12, rng_seed=5, sim_offset=600, counts=acc)
    assert torch.equal(whole, acc)
    assert whole[2, -1].sum().item() > 0
    # the second shard alone is the model's trajectories 600..999
    part = u32(sir_counts(g, seeds, beta, gamma, 40, 12, rng_seed=5, sim_offset=600))
    assert np.array_equal(part, expected("nodes/shard").counts)


def test_extreme_thresholds(dev):
    """p = 1 always fires (its threshold 2^32 does not fit 32 bits), p = 0 never does, and p = 1 - 2^-33, whose threshold
    is 2^32 - 1, is not p = 1: the 64-bit compare of the scalar path."""
    import gnode_oracle as O
    from gnode.ode_nn import sir_counts
    n, seed, sims = 300, 11, 32
    rp, ci, g = graph("er300", n, 600)
    depth = bfs_depth(rp, ci, seed, n)
    comp, ecc = depth >= 0, int(depth.max())
    assert comp.sum() > 200 and ecc >= 4
    T = ecc + 2
    assert T == case("nodes/ones").T
    ones, zeros = np.ones(n), np.zeros(n)
    # beta = 1, gamma = 0: the infection advances one BFS level per step and nobody recovers
    got = u32(sir_counts(g, [seed], ones, zeros, sims, T, rng_seed=3))
    for t in range(1, T):
        assert np.array_equal(got[1, t], np.where(comp & (depth <= t), sims, 0)), t
    assert np.all(got[1, ecc][comp] == sims) and not got[2].any()
    assert np.array_equal(got, expected("nodes/ones").counts)
    assert np.array_equal(u32(sir_counts(g, [seed], ones, zeros, sims, T, rng_seed=3, edge_scan=True)), got)
    # beta = 0: nothing but the seed ever leaves S
    got0 = u32(sir_counts(g, [seed], zeros, np.full(n, 0.3), sims, T, rng_seed=3))
    others = np.arange(n) != seed
    assert np.all(got0[0, 1:][:, others] == sims) and np.all(got0[0, 1:, seed] == 0)
    assert np.array_equal(got0, expected("nodes/zeros").counts)
    # beta = 1 - 2^-33 -> threshold 2^32 - 1: fires unless the coin word is 2^32 - 1
    almost = np.full(n, 1.0 - 2.0 ** -33)
    assert int(O.coin_threshold(almost[0])) == 2 ** 32 - 1 and int(O.coin_threshold(1.0)) == 2 ** 32
    for scan in (False, True):
        gota = u32(sir_counts(g, [seed], almost, np.full(n, 0.3), sims, T, rng_seed=3, edge_scan=scan))
        assert np.array_equal(gota, expected("nodes/almost").counts)


def test_sir_torch_surface(dev):
    """Arrays through the reference-shaped surface: float64 [1, T, n] counts, rates indexed by node id."""
    from gnode.ode_nn import sir_torch
    c = case("nodes/karate")
    G, n, sims, T, seeds, beta, gamma = c.G, c.n, c.sims, c.T, c.start, c.beta, c.gamma
    want = expected("nodes/karate").counts.astype(np.float64)
    assert want[2, -1].sum() > 0
    S, I, R = sir_torch(G, seeds, beta, gamma.tolist(), sims, T, rng_seed=77)
    assert S.shape == (1, T, n) and S.dtype == np.float64
    assert np.array_equal(S[0], want[0]) and np.array_equal(I[0], want[1]) and np.array_equal(R[0], want[2])
    S1, I1, R1 = sir_torch(G, seeds, beta, gamma, sims, T, rng_seed=77, normalize_t0=True)
    want[:, 0] *= sims
    assert np.array_equal(S1[0], want[0]) and np.array_equal(I1[0], want[1]) and np.array_equal(R1[0], want[2])


def test_scalar_path_untouched_after_per_node_calls(dev):
    """No state leaks through the handle or the workspace: a scalar call after per-node calls still equals the oracle."""
    import oracle_c as OC
    from gnode.ode_nn import sir_counts
    n, seeds = 500, [3, 499]
    rp, ci, g = graph("er-small", n, 2500)
    beta, gamma, _ = node_rates("er-small", n, seeds)
    sir_counts(g, seeds, beta, gamma, 64, 10, rng_seed=9)
    sir_counts(g, seeds, beta, 0.2, 64, 10, rng_seed=9, edge_scan=True)
    for scan in (False, True):
        got = u32(sir_counts(g, seeds, 0.3, 0.2, 64, 10, rng_seed=9, edge_scan=scan))
        assert np.array_equal(got, OC.sir_philox(n, rp, ci, seeds, 0.3, 0.2, 64, 10, rng_seed=9))
