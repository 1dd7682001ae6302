"""CPU: the two models of rates that change over time (tests/sir_schedule_model.py, tests/dmp_schedule_model.py) are held to the
constant-rate models they restate, to each other on the tree case, and to closed forms; and the cases of
tests/schedule_cases.py pass their liveness checks before any GPU test reads them."""
import numpy as np
import pytest

import schedule_cases as K
import sir_cases as SC
import sir_model as M
from dmp_schedule_model import dmp_sir_schedule
from sir_init_model import dmp_sir_init, sigma_ratio
from sir_schedule_model import schedule_thresholds, sir_events_schedule


def test_one_phase_and_equal_phases_are_sir_events():
    n, rp, ci, W, G, p = K.tree()
    nnz = len(ci)
    for start in (p, [0, 57]):
        want = M.sir_events(n, rp, ci, start, M.thresholds(W[0], nnz), G[0], 200, 12, 1234, 5)
        THR, TG = schedule_thresholds([W[0]], [G[0]], nnz, n)
        got = sir_events_schedule(n, rp, ci, start, THR, TG, np.zeros(12, np.int32), 200, 12, 1234, 5)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        THR, TG = schedule_thresholds([W[0]] * 3, [G[0]] * 3, nnz, n)
        got = sir_events_schedule(n, rp, ci, start, THR, TG, K.TREE_PHASE, 200, 12, 1234, 5)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert (want[0] > 0).any() and (want[1] > 0).any()


def test_one_phase_and_equal_phases_are_dmp_sir_init_bit_for_bit():
    n, rp, ci, W, G, p = K.tree()
    for dtype in ("float32", "float64"):
        want = dmp_sir_init(rp, ci, W[0], G[0], p, K.TREE_T, dtype)
        assert np.array_equal(dmp_sir_schedule(rp, ci, [W[0]], [G[0]], np.zeros(K.TREE_T, int), p, K.TREE_T, dtype), want)
        assert np.array_equal(dmp_sir_schedule(rp, ci, [W[0]] * 3, [G[0]] * 3, K.TREE_PHASE, p, K.TREE_T, dtype), want)
    assert np.array_equal(dmp_sir_schedule(rp, ci, [W[0]], [G[0]], [0, 0], p, 2), dmp_sir_init(rp, ci, W[0], G[0], p, 2))


def test_monte_carlo_meets_the_stated_recurrence_on_the_tree_and_no_other():
    """20 000 trajectories against the float64 recurrence: within the project's 5-sigma bound; against the variant that takes
    theta_{t+1}'s weight from step t, and against constant rates, far outside it."""
    n, rp, ci, W, G, p = K.tree()
    t_inf, t_rec = K.tree_events()
    cnt = M.counts(t_inf, t_rec, K.TREE_T, hold_row0=False)
    left = float((t_inf > 0).sum()) / float((t_inf != 0).sum())
    right = sigma_ratio(cnt, K.TREE_SIMS, dmp_sir_schedule(rp, ci, W, G, K.TREE_PHASE, p, K.TREE_T, "float64"), slice(1, None))
    wrong = sigma_ratio(cnt, K.TREE_SIMS, dmp_sir_schedule(rp, ci, W, G, K.TREE_PHASE, p, K.TREE_T, "float64", variant="this"), slice(1, None))
    const = sigma_ratio(cnt, K.TREE_SIMS, dmp_sir_init(rp, ci, W[0], G[0], p, K.TREE_T, "float64"), slice(1, None))
    print(f"tree: {left:.3f} of the initially susceptible pairs left S; sigma ratio {right:.2f}, wrong weight {wrong:.1f}, constant {const:.1f}")
    assert left >= 0.25
    assert right <= 5.0
    assert wrong > 5.0 and const > 5.0


def test_an_all_zero_phase_infects_nobody_while_somebody_is_infected():
    c, want = K.case("er-small/seeds"), K.expected("er-small/seeds")
    closed = np.flatnonzero(c.phase == c.closed)
    closed = closed[closed >= 1]
    assert not np.isin(want.t_inf, closed).any()
    cv = want.curves
    assert (cv[:, closed - 1, 1] > 0).any()                       # infected people stood in front of the closed steps
    assert np.isin(want.t_rec, closed).any()                      # and recovered during them


def test_gamma_one_after_gamma_zero_recovers_everybody_at_the_switch():
    c, want = K.case("everybody"), K.expected("everybody")
    s = c.switch
    assert c.phase[s - 1] == 0 and c.phase[s] == 1
    before = (want.t_inf >= 0) & (want.t_inf < s)
    assert before.all()                                           # w = 1: everybody is infected before the switch
    assert (want.t_rec == s).all()
    assert (want.curves[:, s - 1] == (0, c.n, 0)).all() and (want.curves[:, s] == (0, 0, c.n)).all()


@pytest.mark.parametrize("key", [k for k in K.CASES if k != "everybody"])
def test_the_shape_cases_are_live(key):
    K.live_schedule(K.case(key), K.expected(key))
