"""CPU: the start drawn from an initial-state distribution and the baselines' references of tests/sir_init_model.py -- one-hot
rows ignore the coin, `dmp_sir_init` from a one-hot state is the oracle's `dmp_sir`, and on a tree the Monte-Carlo model's
marginals are DMP's, which tells an ignored immune set apart.  tests/test_sir_model.py holds the model to the oracle."""
import numpy as np

import gnode_oracle as O
import sir_model as M
from sir_cases import case, expected
from sir_init_model import dmp_sir_init, sigma_ratio


def test_one_hot_rows_never_depend_on_the_coin_and_mixed_rows_do():
    p = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.25, 0.25], [0, 0.5, 0.5]] * 40, dtype=np.float64)
    tS, tR = M.init_thresholds(p)
    seen = np.zeros((len(p), 3), dtype=np.int64)
    for sim in range(200):
        st = M.draw_initial_state(tS, tR, sim, np.uint64(5), np.uint64(9))
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
        assert np.array_equal(dmp_sir_init(rp, ci, w, gamma, M.one_hot_init(n, seeds), T, dtype), O.dmp_sir(rp, ci, w, gamma, seeds, T, dtype))


def test_tree_marginals_are_dmp_and_an_ignored_immune_set_is_not():
    """On a tree DMP's marginals are exact: 5 000 trajectories from the mixed state lie within the project's per-cell bound
    |count / sims - P| <= 5 (sqrt(P (1 - P) / sims) + 1 / sims), row 0 included (measured: largest ratio 3.02, 0.512 of the
    (node, trajectory) pairs left S).  DMP with pR folded into pS is not within it (the ratio is `sims`: an immune node
    counted susceptible)."""
    c, got = case("cpu/tree"), expected("cpu/tree")
    p, sims, T, counts = c.start, c.sims, c.T, got.counts
    left = 1.0 - counts[0, -1].sum() / (sims * c.n)
    ratio = sigma_ratio(counts, sims, dmp_sir_init(c.rp, c.ci, c.w, c.gamma, p, T, "float64"))
    print(f"tree: {left:.3f} of the (node, trajectory) pairs left S, largest ratio {ratio:.2f}")
    assert left > 0.25
    assert ratio <= 5.0
    folded = np.stack([p[:, 0] + p[:, 2], p[:, 1], np.zeros(c.n)], 1)
    assert sigma_ratio(counts, sims, dmp_sir_init(c.rp, c.ci, c.w, c.gamma, folded, T, "float64")) > 5.0
