"""No GPU: the model of the Monte-Carlo source scores from timed evidence (tests/sir_timed_model.py) -- every kind and the
"before the outbreak" rule on a hand-made event table, the difference-array form against the definition on random events, the
liveness of every case tests/test_gpu_sir_timed.py runs -- and the model against an EXACT forward filter over the 81 states of
a graph with a loop, for three evidence sets that use all five kinds."""
import numpy as np
import pytest

import sir_score_model as Q
import sir_timed_model as TM


def test_every_kind_and_the_rule_before_the_outbreak_on_a_hand_made_table():
    #          node 0: infected at 2, recovers at 4   1: never   2: starts in R   3: starts in I, never recovers
    t_inf = np.asarray([[2, -1, 0, 0]])
    t_rec = np.asarray([[4, -1, 0, -1]])
    T = 7

    def row(v, d, kind):
        return TM.matched(t_inf, t_rec, (v, d, kind), T)[0].astype(int).tolist()

    assert row(0, 0, 0) == [1, 1, 0, 0, 0, 0, 0] and row(0, 0, 1) == [0, 0, 1, 1, 0, 0, 0] and row(0, 0, 2) == [0, 0, 0, 0, 1, 1, 1]
    assert row(0, 0, 3) == [0, 0, 1, 0, 0, 0, 0] and row(0, 0, 4) == [0, 0, 0, 0, 1, 0, 0]
    # read two steps back: the same rows moved by two, and before the outbreak only kind 0 holds
    assert row(0, -2, 0) == [1, 1, 1, 1, 0, 0, 0] and row(0, -2, 1) == [0, 0, 0, 0, 1, 1, 0] and row(0, -2, 2) == [0, 0, 0, 0, 0, 0, 1]
    assert row(0, -2, 3) == [0, 0, 0, 0, 1, 0, 0] and row(0, -2, 4) == [0, 0, 0, 0, 0, 0, 1]
    # further back than T: before the outbreak at every t
    assert row(0, -7, 0) == [1] * 7 and all(row(0, -7, k) == [0] * 7 for k in (1, 2, 3, 4)) and row(0, -100, 0) == [1] * 7
    # never infected: susceptible for ever, no event
    assert row(1, 0, 0) == [1] * 7 and row(1, -3, 0) == [1] * 7 and all(row(1, 0, k) == [0] * 7 for k in (1, 2, 3, 4))
    # an R start, t_inf = t_rec = 0: kinds 2, 3 and 4 at m = 0, kind 2 from then on, never 0 or 1 (but 0 before the outbreak)
    assert row(2, 0, 2) == [1] * 7 and row(2, 0, 3) == [1, 0, 0, 0, 0, 0, 0] == row(2, 0, 4) and row(2, 0, 0) == [0] * 7 == row(2, 0, 1)
    assert row(2, -1, 0) == [1, 0, 0, 0, 0, 0, 0] and row(2, -1, 3) == [0, 1, 0, 0, 0, 0, 0] == row(2, -1, 4) and row(2, -1, 2) == [0] + [1] * 6
    # an I start: kind 3 at m = 0, infected for ever
    assert row(3, 0, 3) == [1, 0, 0, 0, 0, 0, 0] and row(3, 0, 1) == [1] * 7 and row(3, -2, 1) == [0, 0] + [1] * 5 and row(3, 0, 4) == [0] * 7
    # a set: agree and the bin
    records = [(0, 0, 1), (0, -1, 3), (1, 0, 0), (2, -1, 4), (3, 0, 2)]
    assert TM.agree_of(t_inf, t_rec, records, T)[0].tolist() == [1, 2, 2, 3, 1, 1, 1]
    h = TM.hist_of([(t_inf, t_rec)], [records, records[:2]], 5, T)
    assert h.shape == (2, 1, T, 6) and [int(np.flatnonzero(h[0, 0, t])[0]) for t in range(T)] == [1, 2, 2, 3, 1, 1, 1]
    assert [int(np.flatnonzero(h[1, 0, t])[0]) for t in range(T)] == [0, 0, 2, 5, 0, 0, 0]      # (agree * 5) // 2; 5 only for both
    assert TM.hist_of([(t_inf, t_rec)], [records], 2, T)[0, 0, :, :].argmax(-1).tolist() == [0, 0, 0, 1, 0, 0, 0]


def test_the_difference_array_is_the_definition_on_random_events():
    rng = np.random.default_rng(11)
    n, sims = 9, 300
    for T in (1, 2, 5, 12):
        t_inf = rng.integers(-1, T, (sims, n))
        gap = rng.integers(0, T + 1, (sims, n))
        t_rec = np.where((t_inf >= 0) & (rng.random((sims, n)) < 0.6), t_inf + np.where(t_inf == 0, gap, np.maximum(gap, 1)), -1)
        t_rec = np.where(t_rec >= T, -1, t_rec)
        assert ((t_rec == -1) | (t_rec >= t_inf)).all() and ((t_inf == 0) & (t_rec == 0)).any() == (T > 0)
        for size in (1, 4, 25):
            records = [(int(rng.integers(n)), -int(rng.integers(0, T + 3)), int(rng.integers(5))) for _ in range(size)]
            records[0] = (records[0][0], -(T + int(rng.integers(0, 3))), records[0][2])       # at T or beyond: the clamp
            want = TM.agree_of(t_inf, t_rec, records, T)
            assert np.array_equal(TM.agree_by_differences(t_inf, t_rec, records, T), want), (T, records)
            assert want.min() >= 0 and want.max() <= size
            for bins in (1, size, 7):
                assert np.array_equal(TM.hist_by_differences([(t_inf, t_rec)], [records], bins, T), TM.hist_of([(t_inf, t_rec)], [records], bins, T))


def test_observations_pack_and_unpack():
    records = [(3, 0, 1), (1, -2, 3), (3, 0, 2), (3, -2, 4), (0, -9, 0), (1, -2, 0)]
    obs = TM.Observations(5, records)
    assert obs.n == 5 and obs.row_offsets.tolist() == [0, 0, -2, -2, -9] and obs.rows.shape == (5, 5)
    assert sorted(TM.records_of(obs)) == sorted(records)
    assert TM.records_of(obs) == [(3, 0, 1), (3, 0, 2), (1, -2, 3), (3, -2, 4), (1, -2, 0), (0, -9, 0)]


@pytest.mark.parametrize("key,shifts", TM.RUNS)
def test_every_case_of_the_gpu_module_is_live(key, shifts):
    TM.live(key, shifts, None if shifts == "mixed" else 5)


# ------------------------------------------------------------------------------------------------------- the exact chain
def test_the_forward_filter_gives_the_reference_values():
    P = {k: TM.chain_table(TM.CHAIN_SETS[k]) for k in "DFG"}
    assert np.isclose(P["D"][0, 1], 0.4, rtol=0, atol=1e-12)
    assert np.isclose(P["F"][0, 3], 0.1981, rtol=0, atol=5e-5) and np.isclose(P["G"][2, 2], 0.0756, rtol=0, atol=5e-5)
    assert [int((P[k] >= 0.01).sum()) for k in "DFG"] == [14, 18, 5]
    assert {r[2] for k in "DFG" for r in TM.CHAIN_SETS[k]} == {0, 1, 2, 3, 4} and TM.CHAIN_T == 8 != Q.CHAIN_T
    # with no evidence but "v is in its state", the filter is the chain of tests/test_sir_score_model.py
    from test_sir_score_model import chain_table
    snap = [(v, 0, int(Q.CHAIN_OBS[v])) for v in range(Q.CHAIN_N)]
    assert np.allclose(TM.chain_table(snap, Q.CHAIN_T), chain_table(), rtol=0, atol=1e-15)


def test_the_model_agrees_with_the_exact_chain_on_a_graph_with_a_loop():
    sims = 20_000
    TM.check_chain(TM.chain_hist(sims), sims)
