"""CPU: what a direction means to the model of tests/sir_model.py -- the one-way path, a closed form -- and
`gnode.ode_nn.edge_rates`, which puts a matrix into CSR position order (tests/test_gpu_sir_edges.py feeds the GPU through it).
The model itself is held to the oracle by tests/test_sir_model.py."""
import numpy as np
import pytest

from sir_cases import case, er200 as _er200, expected, karate


def test_one_way_path_is_deterministic():
    """w = 1 along i -> i + 1, 0 along i + 1 -> i, nobody recovers: node m + j leaves S at step j in every trajectory,
    nobody below m ever does."""
    c, got = case("cpu/path12"), expected("cpu/path12")
    n, m, sims, T = c.n, 5, c.sims, c.T
    want = np.full(n, -1)
    want[m:] = np.arange(n - m)
    assert np.array_equal(got.t_inf, np.broadcast_to(want, (sims, n)))
    for t in range(1, T):
        assert np.array_equal(got.counts[1, t], np.where((np.arange(n) >= m) & (np.arange(n) - m <= t), sims, 0))
    assert not got.counts[2].any() and np.all(got.t_rec == -1)


def _shuffled_matrix(n, rp, ci, w, seed):
    """scipy COO of the weights with its entries in shuffled order (and the zeros of w left out)."""
    import scipy.sparse as sp
    src = np.repeat(np.arange(n), np.diff(rp))
    order = np.random.default_rng(seed).permutation(len(ci))
    order = order[w[order] != 0.0]
    return sp.coo_matrix((w[order], (src[order], ci[order])), shape=(n, n))


def test_edge_rates_aligns_a_matrix_with_the_csr():
    import scipy.sparse as sp
    from gnode.ode_nn import EdgeRates, edge_rates
    n, rp, ci = _er200()
    rng = np.random.default_rng(3)
    w = rng.uniform(0.05, 0.9, len(ci))
    w[rng.permutation(len(ci))[:len(ci) // 5]] = 0.0                 # absent from the matrix: the directed case
    w[7] = 1.0
    M = _shuffled_matrix(n, rp, ci, w, 4)
    for form in (M, M.tocsr(), M.tocsc()):
        er = edge_rates((rp, ci), form)
        assert isinstance(er, EdgeRates) and er.w.dtype == np.float64 and er.w.flags["C_CONTIGUOUS"]
        assert (er.n, er.nnz) == (n, len(ci)) and np.array_equal(er.w, w)
    # M[u, v] is the weight of the entry in ROW u: the transpose is another array
    assert not np.array_equal(edge_rates((rp, ci), sp.csr_matrix(M.T)).w, w)
    # an array already in CSR order is taken as it is (a copy: the caller's array stays the caller's)
    er = edge_rates((rp, ci), w.tolist())
    assert np.array_equal(er.w, w) and er.w is not w
    # a pattern whose columns are not sorted inside a row
    rp2, ci2 = np.array([0, 2, 4, 6]), np.array([2, 1, 0, 2, 1, 0])
    M2 = sp.coo_matrix(([0.1, 0.2, 0.3, 0.4], ([0, 0, 2, 1], [1, 2, 0, 0])), shape=(3, 3))
    assert np.array_equal(edge_rates((rp2, ci2), M2).w, [0.2, 0.1, 0.4, 0.0, 0.0, 0.3])


def test_edge_rates_from_a_networkx_graph():
    import scipy.sparse as sp
    from gnode.ode_nn import edge_rates
    G, n, rp, ci = karate()
    w = np.random.default_rng(5).uniform(0.0, 1.0, len(ci))
    assert np.array_equal(edge_rates(G, sp.csr_matrix((w, ci, rp), shape=(34, 34))).w, w)


def test_edge_rates_refuses():
    import scipy.sparse as sp
    from gnode.ode_nn import edge_rates
    n, rp, ci = _er200()
    w = np.full(len(ci), 0.3)
    src = np.repeat(np.arange(n), np.diff(rp))
    for what, x in (("negative", -0.1), ("above one", 1.5), ("NaN", float("nan"))):
        bad = w.copy()
        bad[11] = x
        with pytest.raises(ValueError, match="11"):
            edge_rates((rp, ci), bad)
        with pytest.raises(ValueError):
            edge_rates((rp, ci), sp.csr_matrix((bad, ci, rp), shape=(n, n)))
    for shape_bad in (w[:-1], w.reshape(-1, 1), 0.3):
        with pytest.raises(ValueError):
            edge_rates((rp, ci), shape_bad)
    with pytest.raises(ValueError):
        edge_rates((rp, ci), sp.csr_matrix((w, ci, np.append(rp, rp[-1])), shape=(n + 1, n + 1)))
    # a non-zero entry outside the pattern; a stored zero there is nothing
    A = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n)).toarray()
    u, v = np.argwhere((A == 0) & ~np.eye(n, dtype=bool))[0]
    for val, ok in ((0.4, False), (float("nan"), False), (0.0, True)):
        M = sp.coo_matrix((np.append(w, val), (np.append(src, u), np.append(ci, v))), shape=(n, n))
        if ok:
            assert np.array_equal(edge_rates((rp, ci), M).w, w)
        else:
            with pytest.raises(ValueError):
                edge_rates((rp, ci), M)
