"""No GPU: the model of the Monte-Carlo nowcast and forecast from timed evidence (tests/sir_post_model.py) -- acceptance and the
counts on a hand-made event table, the kernels' one counter per set against the definition on random events, the liveness of
every case tests/test_gpu_sir_post.py runs, the `lonely` runs included -- and the model against an EXACT forward filter over
the 81 states of a graph with a loop, per candidate, at five (set, now)."""
import numpy as np
import pytest

import sir_post_model as PM
import sir_timed_model as TM


def test_acceptance_and_counts_on_a_hand_made_table():
    #   trajectory 0: node 0 infected at 2, recovers at 4; 2 starts in R; 3 starts in I   trajectory 1: only 3, recovers at 1: ended
    t_inf = np.asarray([[2, -1, 0, 0], [-1, -1, -1, 0]])
    t_rec = np.asarray([[4, -1, 0, -1], [-1, -1, -1, 1]])
    T, n = 7, 4
    sets = [[(0, 0, 1), (0, -1, 3)], [(1, 0, 0)], [(3, -1, 4)], [(1, -9, 0), (3, -3, 3)]]
    counts, accepted = PM.posterior_of([(t_inf, t_rec)], sets, T, 3, [0, 1, 3], n)
    assert accepted[:, 0].tolist() == [1, 2, 0, 2]                  # set 0: trajectory 0 alone; (1, S): both; 3 recovered at 2: nobody
    assert counts[0, :, 0].tolist() == [[1, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 1]] and counts[0, :, 1].tolist() == [[0, 0, 1, 0], [1, 0, 1, 0], [1, 0, 1, 0]]
    # the trajectory that ended at step 1 keeps its final state at every horizon
    assert counts[1, :, 0].tolist() == [[1, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 1]] and counts[1, :, 1].tolist() == [[0, 0, 1, 1], [1, 0, 1, 1], [1, 0, 1, 1]]
    assert (counts[2] == 0).all() and np.array_equal(counts[3], counts[1])
    # now = 1: trajectory 1 is judged on the step at which it ended; now = 0: the start
    assert PM.posterior_of([(t_inf, t_rec)], [[(3, 0, 4)]], T, 1, [0], n)[1].tolist() == [[1]]
    c0, a0 = PM.posterior_of([(t_inf, t_rec)], [[(3, 0, 3)], [(2, 0, 4), (0, 0, 0)]], T, 0, [0, 6], n)
    assert a0.tolist() == [[2], [1]] and c0[0, 0].tolist() == [[0, 0, 0, 2], [0, 0, 1, 0]] and c0[0, 1].tolist() == [[0, 0, 0, 1], [1, 0, 1, 1]]
    assert PM.end_step(t_inf, t_rec, T).tolist() == [T, 1] and PM.end_step(t_inf[:, :3] * 0 - 1, t_rec[:, :3] * 0 - 1, T).tolist() == [0, 0]


def test_the_counter_is_the_definition_on_random_events():
    rng = np.random.default_rng(19)
    n, sims = 9, 300
    for T in range(1, 13):
        t_inf = rng.integers(-1, T, (sims, n))                      # never-infected nodes among them
        gap = rng.integers(0, T + 1, (sims, n))
        t_rec = np.where((t_inf >= 0) & (rng.random((sims, n)) < 0.6), t_inf + np.where(t_inf == 0, gap, np.maximum(gap, 1)), -1)
        t_rec = np.where(t_rec >= T, -1, t_rec)
        assert ((t_inf == 0) & (t_rec == 0)).any() and ((t_inf == 0) & (t_rec != 0)).any() and (t_inf < 0).any()     # R starts, I starts
        for size in (1, 4, 25):
            records = [(int(rng.integers(n)), -int(rng.integers(0, T + 3)), int(rng.integers(5))) for _ in range(size)]
            records[0] = (records[0][0], -(T + int(rng.integers(0, 3))), records[0][2])       # at T or beyond
            want = TM.agree_of(t_inf, t_rec, records, T)
            for now in range(T):
                assert np.array_equal(PM.agree_now_by_counter(t_inf, t_rec, records, T, now), want[:, now]), (T, now, records)
            assert np.array_equal(TM.agree_by_differences(t_inf, t_rec, records, T), want)     # (the array it is the prefix sum of)


@pytest.mark.parametrize("key,shifts", PM.RUNS)
def test_every_case_of_the_gpu_module_is_live(key, shifts):
    PM.live(key, shifts)


@pytest.mark.parametrize("key", PM.KEYS)
def test_every_lonely_run_is_live(key):
    PM.lonely_live(key)


# ------------------------------------------------------------------------------------------------------- the exact chain
def test_the_filter_at_h_0_is_the_timed_chain_table_and_its_marginals_are_consistent():
    for name, now in PM.CHAIN_RUNS:
        joint, total = PM.chain_posterior(TM.CHAIN_SETS[name], now)
        assert np.allclose(total, TM.chain_table(TM.CHAIN_SETS[name])[:, now], rtol=0, atol=1e-14)
        assert (joint.sum(2) <= total[:, None, None] + 1e-14).all() and (joint >= 0).all()
        # a record "v is in state k at now" pins that node's marginal at h = 0
        for v, d, kind in TM.CHAIN_SETS[name]:
            if d == 0 and kind in (1, 2):
                assert np.allclose(joint[:, 0, kind - 1, v], total, rtol=0, atol=1e-14)
            if d == 0 and kind == 0:
                assert (joint[:, 0, :, v] == 0).all()
        assert (np.diff(joint[:, :, 1, :], axis=1) >= -1e-14).all()  # removal only grows with the horizon
    assert PM.chain_posterior(TM.CHAIN_SETS["D"], 0)[1].max() == 0.0
    assert np.isclose(PM.chain_posterior(TM.CHAIN_SETS["D"], 1)[1][0], 0.4, rtol=0, atol=1e-12)
    # no evidence at all: the unconditional marginals of the chain
    free, one = PM.chain_posterior(((3, -(TM.CHAIN_T + 1), 0),), 2, (0, 1))
    states, M = TM.chain_matrix()
    x = np.zeros(81); x[states.index((0, 1, 0, 0))] = 1.0
    x = x @ M @ M
    assert np.allclose(one, 1.0) and np.isclose(free[1, 0, 0, 1], x[np.asarray(states)[:, 1] == 1].sum(), rtol=0, atol=1e-14)


def test_the_model_agrees_with_the_exact_chain_per_candidate():
    worst, cells = 0.0, 0
    for name, now in PM.CHAIN_RUNS:
        counts, accepted = PM.chain_counts(name, now)
        share, k = PM.check_chain(name, now, counts, accepted)
        worst, cells = max(worst, share), cells + k
        if (name, now) == ("D", 0):
            assert accepted.sum() == 0 and counts.sum() == 0
        else:
            assert accepted.sum() > 0
    print("largest share of the bound", worst, "cells with P >= 0.01", cells)
    assert worst <= 1.0 and cells == 128
