"""CPU: tests/meanfield_rates_model.py, the float64 yardstick of the GPU tests, against the vectors the reference's own
`runge_kutta_order4` wrote for a weighted, partly directed contact network and for per-node beta
(tests/golden/make_golden_meanfield_rates.py; LSODA at its default tolerances) at the project's 1e-6 mean-field bar.
Measured max |model - reference|: karate 1.952e-08, er150 3.537e-08."""
import numpy as np
import pytest

from meanfield_rates_model import MF_ATOL, golden_case, in_weight_matrix, max_diff, meanfield_rates, one_hot


@pytest.mark.parametrize("name", ["karate", "er150"])
def test_model_matches_reference_vectors(name):
    d = golden_case(name)
    n = len(d["rowptr"]) - 1
    got = meanfield_rates(d["rowptr"], d["col"], one_hot(n, d["seeds"]), d["beta"], d["w"], d["gamma"], d["maxTime"], d["deltaT"])
    want = (d["I"], d["S"], d["R"])
    diff = max_diff(got, want)
    print(f"meanfield rates model {name}: max |model - reference| = {diff:.3e}")
    for g, w in zip(got, want):
        assert g.shape == w.shape == (d["maxTime"], n)
    assert diff <= MF_ATOL
    assert want[0][-1].max() > 1000 * MF_ATOL                        # the epidemic is there to be compared


def test_golden_cases_are_what_the_issue_asks():
    k, e = golden_case("karate"), golden_case("er150")
    assert k["beta"] is None and k["w"].shape == k["col"].shape and k["gamma"].shape == (34,)
    pos = k["w"][k["w"] > 0]
    assert 0.02 <= pos.min() and pos.max() <= 0.15 and 0.1 <= k["gamma"].min() and k["gamma"].max() <= 0.5
    assert (k["w"] == 0).sum() == (len(k["col"]) // 2) // 5          # a fifth of the edges are one-way
    Mt = in_weight_matrix(k["rowptr"], k["col"], k["w"]).toarray()
    assert ((Mt == 0) & (Mt.T > 0)).sum() == (k["w"] == 0).sum()    # ... and their forward entries transmit
    assert e["w"] is None and e["beta"].shape == (150,) and 0.02 <= e["beta"].min() and e["beta"].max() <= 0.1
    assert np.all(e["gamma"] == 0.4) and e["deltaT"] == 0.5 and e["maxTime"] == 15 and k["maxTime"] == 20


def test_in_weights_are_the_transpose():
    rp, ci = np.array([0, 1, 3, 4]), np.array([1, 0, 2, 1])          # path 0 - 1 - 2
    w = np.array([0.5, 0.0, 0.5, 0.0])                               # 0 -> 1 -> 2 only
    I, S, R = meanfield_rates(rp, ci, one_hot(3, [2]), None, w, 0.2, 6)
    assert np.array_equal(S[:, :2], np.ones((6, 2))) and not I[:, :2].any()
    I, S, R = meanfield_rates(rp, ci, one_hot(3, [0]), None, w, 0.2, 6)
    assert I[-1, 2] > 1e-3
