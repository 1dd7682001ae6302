"""CPU: the yardstick of the scheduled DMP gradients (tests/dmp_schedule_grad_model.py) is itself held to something -- its
float64 forward to the scheduled reference tests/dmp_schedule_model.dmp_sir_schedule (equal outputs), its gradients to central
differences in float64, and a schedule that changes nothing to tests/dmp_grad_model.py's gradients summed over the phases.  The
last test shows that the GPU tests' bar can see the mistake it is there for: theta_{t+1}'s weight gradient given to step t's
table lies 1e-1 .. 6e-1 from the truth wherever there is an edge pass."""
import numpy as np
import pytest

import dmp_grad_model as M
import dmp_schedule_grad_model as S
from baseline_cases import rel as _rel
from dmp_schedule_model import dmp_sir_schedule

CASES = [("er300_T2", "mixed"), ("er300_T3", "mixed"), ("er300_T8", "mixed"), ("er300_T8", "seeds"), ("er34", "mixed"),
         ("isolated", "mixed"), ("nnz0", "mixed")]
IDS = [f"{n}-{s}" for n, s in CASES]


def test_phases_are_spread_and_phase_zero_comes_back():
    assert S.spread_phases(2).tolist() == [0, 1] and S.spread_phases(3).tolist() == [0, 1, 0]
    for T in (4, 7, 8, 10, 12):
        p = S.spread_phases(T)
        assert p.dtype == np.int32 and len(p) == T and p[T - 1] == 0 and p[1] == 0
        assert sorted(set(p[1:T - 1].tolist())) == [0, 1, 2][:min(3, T - 2)] and (np.diff(p[1:T - 1]) >= 0).all()
    assert S.spread_phases(8, P=7).tolist() == [0, 0, 1, 2, 3, 4, 5, 0]


@pytest.mark.parametrize("name,start", CASES, ids=IDS)
def test_float64_forward_equals_the_scheduled_reference(name, start):
    c = S.case(name, start)
    ref = dmp_sir_schedule(c["rp"], c["ci"], c["W"], c["Gam"], c["phase"], c["init"], c["T"], "float64")
    assert np.array_equal(S.model(name, start, "float64")[0], ref)
    lo = S.model(name, start, "float32")[0]
    assert _rel(lo, ref) <= 1e-5


@pytest.mark.parametrize("name,start", CASES, ids=IDS)
def test_gradients_are_the_central_differences(name, start):
    """The derivative of sum(grad_out * out) along three random directions per input, float64, step 1e-6: the truncation error is
    O(h^2) = 1e-12 relative and the rounding error about 1e-16 / h = 1e-10, so 1e-7 of the gradient's scale is a wide bound."""
    c = S.case(name, start)
    hi = S.model(name, start, "float64")
    rng = np.random.default_rng(11)
    x0 = [np.asarray(c[k], dtype=np.float64) for k in ("W", "Gam", "init")]

    def loss(x):
        import torch
        src, rev = (torch.from_numpy(a) for a in M.tables(c["rp"], c["ci"]))
        out = S.forward(src, rev, len(c["rp"]) - 1, torch.from_numpy(x[0]), torch.from_numpy(x[1]), c["phase"], torch.from_numpy(x[2]), c["T"])
        return float((out * torch.from_numpy(c["G"].astype(np.float64))).sum())

    h = 1e-6
    for i, key in enumerate(("W", "gamma", "init")):
        if x0[i].size == 0:
            continue
        for _ in range(3):
            d = rng.standard_normal(x0[i].shape)
            up, dn = [a.copy() for a in x0], [a.copy() for a in x0]
            up[i] += h * d
            dn[i] -= h * d
            fd, an = (loss(up) - loss(dn)) / (2 * h), float((hi[1 + i] * d).sum())
            scale = float(np.abs(hi[1 + i]).max() * np.abs(d).sum()) or 1.0
            assert abs(fd - an) <= 1e-7 * scale, f"{name}/{start} d/d{key}: {fd} vs {an}"


@pytest.mark.parametrize("name,start", CASES, ids=IDS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_schedule_that_changes_nothing_is_the_constant_model(name, start, dtype):
    """One phase gives dmp_grad_model.gradients, and three phases holding equal tables give it summed over the phases: the
    outputs bit for bit, the gradients up to the order of autograd's additions.  An entry of a table's gradient is a sum of at
    most 2 (T - 1) terms, one or two per step; both models add the same terms, the scheduled one through an index per step and
    then over the phases, so the two sums differ by at most about 2 T eps times the terms' magnitude: 64 eps of the tensor's
    largest entry is held here (T <= 12)."""
    c = S.case(name, start)
    want = M.gradients(c["rp"], c["ci"], c["w"], c["gam"], c["init"], c["T"], c["G"], dtype)
    one = S.gradients(c["rp"], c["ci"], c["w"][None], c["gam"][None], np.zeros(c["T"], int), c["init"], c["T"], c["G"], dtype)
    same = S.gradients(c["rp"], c["ci"], np.stack([c["w"]] * 3), np.stack([c["gam"]] * 3), c["phase"], c["init"], c["T"], c["G"], dtype)
    eps = float(np.finfo(dtype).eps)
    for got in (one, same):
        assert np.array_equal(got[0], want[0])
        for a, b in zip((got[1].sum(0), got[2].sum(0), got[3]), want[1:]):
            assert a.shape == b.shape
            if b.size:
                assert np.abs(a - b).max() <= 64 * eps * max(float(np.abs(b).max()), 1e-30)


@pytest.mark.parametrize("name,start", CASES, ids=IDS)
def test_the_bar_sees_a_weight_gradient_given_to_the_wrong_step(name, start):
    c = S.case(name, start)
    hi = S.model(name, start, "float64")
    wrong = S.gradients(c["rp"], c["ci"], c["W"], c["Gam"], c["phase"], c["init"], c["T"], c["G"], "float64", attribution="this")
    assert np.array_equal(wrong[0], hi[0]) and np.array_equal(wrong[2], hi[2]) and np.array_equal(wrong[3], hi[3])
    if c["T"] >= 3 and len(c["ci"]):
        assert _rel(wrong[1], hi[1]) >= 6e-2                        # four orders above the bar's max(4 yard, 1e-6)
    else:                                                           # no edge pass: nothing to attribute
        assert np.array_equal(wrong[1], hi[1])
    if c["T"] == 2 and len(c["ci"]):                                # theta_1 alone: only phase[1]'s table has a gradient
        assert hi[1][int(c["phase"][1])].any() and not np.delete(hi[1], int(c["phase"][1]), axis=0).any()
