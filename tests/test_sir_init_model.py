"""CPU: the models of tests/sir_init_model.py (initial-state distributions) are held to the oracle -- a one-hot state is the
seed-list model, and on a tree the Monte-Carlo's marginals are DMP's, which tells an ignored immune set apart."""
import numpy as np

import gnode_oracle as O
from sir_edges_model import sir_philox_edges
from sir_init_model import dmp_sir_init, one_hot_init, sigma_ratio, sir_philox_init, tree_init


def test_one_hot_init_is_the_seed_list_model():
    n, sims, T, seeds = 203, 40, 10, [3, 77, 202]
    rp, ci, _ = O.er_graph(n, 700, seed=4)
    p = one_hot_init(n, seeds)
    want = O.sir_philox(n, rp, ci, seeds, 0.3, 0.2, sims, T, rng_seed=17, sim_offset=3)
    got = sir_philox_init(n, rp, ci, p, 0.3, 0.2, sims, T, 17, sim_offset=3)
    assert want[1, 1:].any() and want[2, 1:].any()
    assert np.array_equal(got[:, 1:], want[:, 1:]) and np.array_equal(got[:, 0], sims * want[:, 0])
    rng = np.random.default_rng(6)
    w, gamma = rng.uniform(0.05, 0.9, len(ci)), rng.uniform(0.05, 0.6, n)
    w[rng.permutation(len(ci))[:len(ci) // 5]] = 0.0
    want, wi, wr = sir_philox_edges(n, rp, ci, seeds, w, gamma, sims, T, 18, 2, return_events=True)
    got, gi, gr = sir_philox_init(n, rp, ci, p, w, gamma, sims, T, 18, 2, return_events=True)
    assert np.array_equal(got[:, 1:], want[:, 1:]) and np.array_equal(got[:, 0], sims * want[:, 0])
    assert np.array_equal(gi, wi) and np.array_equal(gr, wr)


def test_one_hot_rows_never_depend_on_the_coin_and_mixed_rows_do():
    from sir_init_model import draw_initial_state, init_thresholds
    p = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.25, 0.25], [0, 0.5, 0.5]] * 40, dtype=np.float64)
    tS, tR = init_thresholds(p)
    seen = np.zeros((len(p), 3), dtype=np.int64)
    for sim in range(200):
        st = draw_initial_state(tS, tR, sim, np.uint64(5), np.uint64(9))
        seen[np.arange(len(p)), st] += 1
    assert np.all(seen[0::5] == [200, 0, 0]) and np.all(seen[1::5] == [0, 200, 0]) and np.all(seen[2::5] == [0, 0, 200])
    assert not seen[4::5, 0].any()
    f = seen[3::5].sum(0) / seen[3::5].sum()                       # 8 000 draws: 5 sigma of a proportion
    assert np.all(np.abs(f - [0.5, 0.25, 0.25]) <= 5 * np.sqrt(0.25 / 8000))


def test_dmp_one_hot_is_the_oracle_bit_for_bit():
    n, seeds, T = 150, [4, 90], 9
    rp, ci, _ = O.er_graph(n, 400, seed=2)
    rng = np.random.default_rng(3)
    w, gamma = rng.uniform(0.05, 0.5, len(ci)), rng.uniform(0.1, 0.5, n)
    for dtype in ("float32", "float64"):
        assert np.array_equal(dmp_sir_init(rp, ci, w, gamma, one_hot_init(n, seeds), T, dtype), O.dmp_sir(rp, ci, w, gamma, seeds, T, dtype))


def test_tree_marginals_are_dmp_and_an_ignored_immune_set_is_not():
    """On a tree DMP's marginals are exact: 5 000 trajectories from the mixed state lie within the project's per-cell bound
    |count / sims - P| <= 5 (sqrt(P (1 - P) / sims) + 1 / sims), row 0 included (measured: largest ratio 3.02, 0.512 of the
    (node, trajectory) pairs left S).  DMP with pR folded into pS is not within it (the ratio is `sims`: an immune node
    counted susceptible)."""
    from test_gpu_sir_edges import tree_case
    n, rp, ci, w, gamma = tree_case()
    p, sims, T = tree_init(), 5000, 12
    counts = sir_philox_init(n, rp, ci, p, w, gamma, sims, T, 1234)
    left = 1.0 - counts[0, -1].sum() / (sims * n)
    ratio = sigma_ratio(counts, sims, dmp_sir_init(rp, ci, w, gamma, p, T, "float64"))
    print(f"tree: {left:.3f} of the (node, trajectory) pairs left S, largest ratio {ratio:.2f}")
    assert left > 0.25
    assert ratio <= 5.0
    folded = np.stack([p[:, 0] + p[:, 2], p[:, 1], np.zeros(n)], 1)
    assert sigma_ratio(counts, sims, dmp_sir_init(rp, ci, w, gamma, folded, T, "float64")) > 5.0
