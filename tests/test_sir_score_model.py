"""No GPU: the model of the Monte-Carlo source scores (tests/sir_score_model.py) -- every cell of the histogram holds sims
trajectories, the snapshot taken from a trajectory finds it again in the top bin, the two measures are their set definitions
on a hand-made case, the liveness of every case tests/test_gpu_sir_score.py runs -- and the model against an EXACT Markov
chain on a graph with a loop, a 3^n-state transition matrix in float64 written out here."""
import itertools

import numpy as np
import pytest

import sir_score_model as Q


def test_the_measures_and_the_bin_on_a_hand_made_state():
    #                 node  0  1  2  3  4  5  6
    state = np.asarray([[0, 1, 2, 1, 0, 2, 0]], dtype=np.int8)
    obs = np.asarray([[0, 1, 1, 0, -1, -1, 2],       # A = {1, 2, 6}, B = {1, 2, 3}: 2 / 4; agree {0, 1}: 2 / 5
                      [0, 1, 2, 1, 0, 2, 0],         # the state itself
                      [0, 0, 0, 0, -1, -1, 0],       # A empty, B = {1, 2, 3}: 0 / 3; agree {0, 6}: 2 / 5
                      [-1, -1, -1, -1, 0, -1, 0]],   # A and B empty: 0 / 0, the top bin; agree 2 / 2
                     dtype=np.int8)
    assert Q.similarity_bins(state, obs, "jaccard", 64)[:, 0].tolist() == [32, 64, 0, 64]
    assert Q.similarity_bins(state, obs, "match", 64)[:, 0].tolist() == [(2 * 64) // 5, 64, (2 * 64) // 5, 64]
    assert Q.similarity_bins(state, obs, "jaccard", 7)[:, 0].tolist() == [3, 7, 0, 7]
    assert Q.bin_of([0, 3, 5, 5], [0, 5, 5, 0], 7).tolist() == [7, 4, 7, 7]


@pytest.mark.parametrize("key,measure,bins,shifts", Q.RUNS)
def test_every_case_of_the_gpu_module_is_live(key, measure, bins, shifts):
    """sum_k hist = sims in every (o, c, t); snapshot (a) puts its trajectory into the top bin of its candidate at its step"""
    Q.live(key, measure, bins, shifts)


@pytest.mark.parametrize("measure", sorted(Q.MEASURES))
def test_the_snapshot_of_a_trajectory_finds_it_in_the_top_bin(measure):
    c = Q.case("er-small/init")
    for shifts in ("mixed", "zeros"):
        h = Q.expected("er-small/init", measure, 64, shifts)
        t_inf, t_rec = Q.case_events("er-small/init", shifts)[2]
        state = Q.states_at(t_inf, t_rec, c.T // 2)
        obs = Q.snapshots("er-small/init", shifts)
        assert np.array_equal(state[0], obs[0])                     # the trajectory that made it is in the sample
        assert h[0, 2, c.T // 2, 64] == (state == obs[0]).all(1).sum() >= 1
        assert (h.sum(-1) == c.sims).all()


def test_the_kernel_of_a_histogram():
    h = np.zeros((2, 3, 5), dtype=np.uint64)                        # [C = 2, T = 3, bins + 1 = 5]
    h[0, 0, 4], h[0, 1, 2], h[0, 1, 4], h[1, 2, 0] = 10, 4, 6, 10
    s = Q.kernel_scores(h, 10, width=0.5, floor=1e-30)
    assert s[0, 0] == 0.0 and np.isclose(s[0, 1], np.log(0.4 * np.exp(-1.0) + 0.6)) and np.isclose(s[1, 2], -4.0)
    assert s[1, 0] == np.log(1e-30)


# ------------------------------------------------------------------------------------------------------- the exact chain
def chain_table():
    """float64 [4, T]: P(state at step t == CHAIN_OBS | node c alone infected at step 0), by the 81-state transition matrix:
    on the pre-step state, a susceptible node with k infected neighbours is infected with probability 1 - (1 - w)^k and an
    infected node recovers with probability gamma, independently"""
    n, w, gamma = Q.CHAIN_N, Q.CHAIN_W, Q.CHAIN_GAMMA
    nb = [[] for _ in range(n)]
    for u, v in Q.CHAIN_EDGES:
        nb[u].append(v); nb[v].append(u)
    states = list(itertools.product(range(3), repeat=n))
    index = {s: i for i, s in enumerate(states)}
    M = np.zeros((len(states), len(states)))
    for s in states:
        per_node = []                                               # [(next state, probability)] of each node
        for v in range(n):
            if s[v] == 0:
                q = 1.0 - (1.0 - w) ** sum(s[u] == 1 for u in nb[v])
                per_node.append([(0, 1.0 - q), (1, q)])
            elif s[v] == 1:
                per_node.append([(1, 1.0 - gamma), (2, gamma)])
            else:
                per_node.append([(2, 1.0)])
        for combo in itertools.product(*per_node):
            M[index[s], index[tuple(x for x, _ in combo)]] += np.prod([p for _, p in combo])
    assert np.allclose(M.sum(1), 1.0, rtol=0, atol=1e-15)
    target = index[tuple(int(x) for x in Q.CHAIN_OBS)]
    P = np.zeros((n, Q.CHAIN_T))
    for c in range(n):
        x = np.zeros(len(states))
        x[index[tuple(int(v == c) for v in range(n))]] = 1.0
        for t in range(Q.CHAIN_T):
            P[c, t] = x[target]
            x = x @ M
    return P


def check_chain(hist, sims, P):
    """the comparison of the issue, on a histogram uint64 [4, T, bins + 1] of the chain's snapshot under "match\""""
    bins = hist.shape[-1] - 1
    est = hist[:, :, bins].astype(np.float64) / sims
    share = np.abs(est - P) / Q.chain_bound(P, sims)
    print("P =", np.round(P, 4).tolist())
    print("estimate =", np.round(est, 4).tolist())
    print("largest share of the bound:", float(share.max()), "at", np.unravel_index(share.argmax(), share.shape))
    assert (hist.sum(-1) == sims).all()
    assert (P >= 0.01).sum() >= 10
    assert (share <= 1.0).all()
    assert (hist[:, :, bins][P == 0.0] == 0).all() and (P[3] == 0.0).all() and (P[:, 0] == 0.0).all()
    assert np.unravel_index(est.argmax(), est.shape) == (0, 2) == np.unravel_index(P.argmax(), P.shape)


def test_the_model_agrees_with_the_exact_chain_on_a_graph_with_a_loop():
    P = chain_table()
    assert np.isclose(P[0, 2], 0.1045, atol=5e-5) and np.isclose(P[0, 3], 0.0847, atol=5e-5) and (P >= 0.01).sum() == 11
    sims = 20_000
    check_chain(Q.chain_hist(sims), sims, P)
