"""CPU: the float64 restatement of the ODEBlock input gradient (oracle/gnode_restate.py adjoint's "x") against x.grad of the
reference's own classes (tests/golden/input_grad_*.npz, make_golden_input_grad.py) -- Euler and RK4, one and many samples,
H = 8 .. 128, hub rows of real fb-social, the eight-graph batch with its marker column -- to float64 rounding; the columns
past gamma are 0."""
import numpy as np
import pytest

import fixture_cases as FC
import gnode_restate as RS

CASES = ["input_grad_karate_B2_H64_T20", "input_grad_loops40_B3_H8_T5", "input_grad_er200_B2_H48_T6",
         "input_grad_er200_B2_H128_T4", "input_grad_fbsocial_B1_H64_T30", "input_grad_multi8_H8_T20",
         "input_grad_rk4_karate_B2_H64_T20"]


@pytest.mark.parametrize("name", CASES)
def test_restated_input_gradient_matches_reference(name):
    d = FC.load(name)
    args = FC.restate_args(d)
    x2d, gx = args[0], RS.adjoint(*args, method=str(d["method"]))["x"]
    assert gx.shape == x2d.shape
    for c in (slice(0, 3), slice(3, 5)):
        want = d["GX"][:, c]
        err = np.abs(gx[:, c] - want).max() / np.abs(want).max()
        assert err <= 1e-9, (name, c, err)
    assert np.abs(gx[:, 5:]).max() == 0.0 and float(d["rest_max"]) == 0.0
    assert np.abs(d["GX"][:, 3:5]).max() > 0                          # beta / gamma do move the loss
    assert all(0 < v < 5e-5 for v in d["yard32"])                       # the fp32 yardstick sits well under the GPU tolerance


def test_restatement_is_sensitive_to_the_beta_gamma_rule():
    """Dropping the stage weights' middle terms (the Euler rule on an RK4 trajectory) misses the RK4 fixture by far more
    than the GPU tolerance: the fixtures do tell the rules apart."""
    d = FC.load("input_grad_rk4_karate_B2_H64_T20")
    gx = RS.adjoint(*FC.restate_args(d), method="euler")["x"]
    err = np.abs(gx[:, 3:5] - d["GX"][:, 3:5]).max() / np.abs(d["GX"][:, 3:5]).max()
    assert err > 1e-2, err
