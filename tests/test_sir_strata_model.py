"""No GPU: the model of the Monte-Carlo nowcast from evidence that may be wrong (tests/sir_strata_model.py) -- the liveness of
every case tests/test_gpu_sir_strata.py runs, the `lonely` runs included, stratum 0 against tests/sir_post_model.py, the
kernels' reading of the counter against the definition on random events -- and the model against an EXACT forward filter with a
mismatch counter over the 81 states of a graph with a loop, per candidate, at five (set, now)."""
import numpy as np
import pytest

import sir_post_model as PM
import sir_strata_model as XM
import sir_timed_model as TM


def test_strata_on_a_hand_made_table():
    #   trajectory 0: node 0 infected at 2, recovers at 4; 2 starts in R; 3 starts in I   trajectory 1: only 3, recovers at 1: ended
    t_inf = np.asarray([[2, -1, 0, 0], [-1, -1, -1, 0]])
    t_rec = np.asarray([[4, -1, 0, -1], [-1, -1, -1, 1]])
    T, n = 7, 4
    sets = [[(0, 0, 1), (0, -1, 3)], [(1, 0, 0)], [(3, -1, 4), (1, -9, 1)]]
    counts, accepted = XM.strata_of([(t_inf, t_rec)], sets, T, 3, [0, 1, 3], n, 2)
    # set 0: trajectory 0 matches both, trajectory 1 neither; set 1: both match; set 2: 3 recovered at 1, not 2, and nobody is infected before the outbreak
    assert accepted[:, 0].tolist() == [[1, 0, 1], [2, 0, 0], [0, 0, 2]]
    assert counts[0, 0, :, 0].tolist() == [[1, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 1]] and counts[0, 2, :, 1].tolist() == [[0, 0, 0, 1]] * 3
    assert (counts[0, 1] == 0).all() and (counts[0, 2, :, 0] == 0).all() and np.array_equal(counts[2, 2], counts[1, 0])
    want = PM.posterior_of([(t_inf, t_rec)], sets, T, 3, [0, 1, 3], n)
    assert np.array_equal(counts[:, 0], want[0]) and np.array_equal(accepted[:, :, 0], want[1])
    # M = 0 is the exact-match posterior; a smaller M is a prefix
    c0, a0 = XM.strata_of([(t_inf, t_rec)], sets, T, 3, [0, 1, 3], n, 0)
    assert np.array_equal(c0, counts[:, :1]) and np.array_equal(a0, accepted[:, :, :1])


@pytest.mark.parametrize("key,shifts", XM.RUNS)
def test_every_case_of_the_gpu_module_is_live(key, shifts):
    XM.live(key, shifts)


@pytest.mark.parametrize("key,shifts", XM.RUNS)
def test_stratum_0_is_the_posterior_model(key, shifts):
    counts, accepted = XM.expected(key, shifts)
    want_counts, want_accepted = PM.expected(key, shifts)
    assert np.array_equal(counts[:5, 0], want_counts) and np.array_equal(accepted[:5, :, 0], want_accepted)


@pytest.mark.parametrize("key", XM.KEYS)
def test_every_lonely_run_is_live(key):
    XM.lonely_live(key)


def test_the_counter_gives_the_strata_on_random_events():
    rng = np.random.default_rng(23)
    n, sims = 9, 300
    for T in range(1, 13):
        t_inf = rng.integers(-1, T, (sims, n))                      # never-infected nodes among them
        gap = rng.integers(0, T + 1, (sims, n))
        t_rec = np.where((t_inf >= 0) & (rng.random((sims, n)) < 0.6), t_inf + np.where(t_inf == 0, gap, np.maximum(gap, 1)), -1)
        t_rec = np.where(t_rec >= T, -1, t_rec)
        for size in (1, 4, 25):
            records = [(int(rng.integers(n)), -int(rng.integers(0, T + 3)), int(rng.integers(5))) for _ in range(size)]
            records[0] = (records[0][0], -(T + int(rng.integers(0, 3))), records[0][2])       # at T or beyond
            for now in range(T):
                d = XM.missed_of(t_inf, t_rec, records, T, now)
                assert np.array_equal(XM.strata_by_counter(t_inf, t_rec, records, T, now), d), (T, now, records)
                assert d.min() >= 0 and d.max() <= size


# ------------------------------------------------------------------------------------------------------- the exact chain
def test_the_filter_with_a_counter_is_consistent():
    """stratum 0 is tests/sir_post_model.py's filter; with every record covered (M = R = 3) the strata of a candidate sum to 1
    and their joint marginals to the chain's unconditional ones"""
    states, P = TM.chain_matrix()
    code = np.asarray(states)
    for name, now in XM.CHAIN_RUNS:
        joint, total = XM.chain_strata(TM.CHAIN_SETS[name], now, XM.CHAIN_M)
        want_joint, want_total = PM.chain_posterior(TM.CHAIN_SETS[name], now)
        assert np.allclose(joint[:, 0], want_joint, rtol=0, atol=1e-14) and np.allclose(total[:, 0], want_total, rtol=0, atol=1e-14)
        assert np.allclose(total.sum(1), 1.0, rtol=0, atol=1e-13) and (joint >= 0).all()
        assert (joint.sum(3) <= total[:, :, None, None] + 1e-14).all()
        for c in range(4):
            x = np.zeros(81); x[states.index(tuple(int(v == c) for v in range(4)))] = 1.0
            x = x @ np.linalg.matrix_power(P, now + 1)
            for v in range(4):
                assert np.isclose(joint[c, :, 1, 0, v].sum(), x[code[:, v] == 1].sum(), rtol=0, atol=1e-13)
        # a smaller M is a prefix of the same filter
        j1, t1 = XM.chain_strata(TM.CHAIN_SETS[name], now, 1)
        assert np.array_equal(j1, joint[:, :2]) and np.array_equal(t1, total[:, :2])
    # (D, 0): two records are read at step 0 of which the candidate matches at most ... and one before the outbreak, kind 1: never matched
    assert XM.chain_strata(TM.CHAIN_SETS["D"], 0, 3)[1][:, 0].max() == 0.0


def test_the_model_agrees_with_the_exact_chain_per_candidate():
    worst, cells = 0.0, 0
    for name, now in XM.CHAIN_RUNS:
        counts, accepted = XM.chain_counts(name, now)
        assert (accepted.sum(1) == XM.CHAIN_SIMS).all()             # every set is complete at M = 3
        share, k = XM.check_chain(name, now, counts, accepted)
        worst, cells = max(worst, share), cells + k
    print("largest share of the bound", worst, "cells with P >= 0.01", cells)
    assert worst <= 1.0 and cells == 1060                           # (the largest share is 0.683 with the model's seed)
