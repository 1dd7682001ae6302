"""CPU: the yardstick of the differentiable DMP baseline (tests/dmp_grad_model.py) is itself held to two things: its float64
forward is the float64 restatement of the recurrence that the forward kernels are held to (sir_init_model.dmp_sir_init), exactly;
and its float64 gradient is the derivative, by central differences along a random direction per input."""
import numpy as np
import pytest

import dmp_grad_model as M


@pytest.mark.parametrize("name", ["er34", "er300_T3", "isolated", "nnz0"])
@pytest.mark.parametrize("start", ["mixed", "seeds"])
def test_float64_forward_is_the_restatement(name, start):
    from sir_init_model import dmp_sir_init
    c = M.case(name, start)
    want = dmp_sir_init(c["rp"], c["ci"], c["w"], c["gam"], c["init"], c["T"], "float64")
    got = M.model(name, start, "float64")[0]
    assert got.shape == want.shape and np.isfinite(want).all()
    diff = float(np.max(np.abs(got - want)))
    print(f"{name}/{start}: max |model - dmp_sir_init| = {diff:.1e}")
    assert diff == 0.0


def test_float64_gradient_is_the_derivative():
    """er(34, 78, 3), T = 12, a third of the weights 0, gamma at 0 and at 1, a mixed start: d/dh sum(G * out(x + h d)) at h = 0 by
    central differences with h = 1e-6 against <grad, d>, per input, to 1e-7 relative (the differences' own error is
    ~h^2 |f'''| + eps / h ~ 1e-10 relative here)."""
    c = M.case("er34", "mixed")
    x = dict(w=c["w"].astype(np.float64), gam=c["gam"].astype(np.float64), init=c["init"].astype(np.float64))
    assert (x["w"] == 0.0).sum() >= len(x["w"]) // 3 and (x["gam"] == 0.0).any() and (x["gam"] == 1.0).any()
    _, *grads = M.model("er34", "mixed", "float64")
    G = c["G"].astype(np.float64)

    def loss(**moved):
        a = dict(x, **moved)
        return float((M.gradients(c["rp"], c["ci"], a["w"], a["gam"], a["init"], c["T"], G)[0] * G).sum())

    h = 1e-6
    for i, (key, grad) in enumerate(zip(("w", "gam", "init"), grads)):
        d = np.random.default_rng(100 + i).standard_normal(x[key].shape)
        fd = (loss(**{key: x[key] + h * d}) - loss(**{key: x[key] - h * d})) / (2 * h)
        an = float((grad * d).sum())
        print(f"{key}: central difference {fd:.12e}, gradient {an:.12e}, relative {abs(fd - an) / abs(fd):.1e}")
        assert abs(fd) > 1e-3 and abs(fd - an) <= 1e-7 * abs(fd)


def test_model_takes_what_dmp_marginals_takes():
    """The model is the yardstick of `gnode.dmp.dmp_marginals`: the same inputs in the same order after the graph, and the
    weights in the CSR position order that `DmpGraph` keeps."""
    import inspect
    import scipy.sparse as sp
    from gnode.dmp import DmpGraph, dmp_marginals
    assert list(inspect.signature(dmp_marginals).parameters) == ["graph", "weights", "gamma", "init", "maxTime"]
    assert list(inspect.signature(M.gradients).parameters)[2:6] == ["w", "gamma", "init", "T"]
    c = M.case("er34", "mixed")
    n = len(c["rp"]) - 1
    data = c["w"].astype(np.float64) + 1.0                          # (no zero: a matrix made elsewhere may drop those)
    G = DmpGraph(sp.csr_matrix((data, c["ci"], c["rp"]), shape=(n, n)))
    assert np.array_equal(G.indptr, c["rp"]) and np.array_equal(G.indices, c["ci"]) and np.array_equal(G.data, data)


def test_yard_is_below_the_projects_cap():
    """The bar of tests/test_gpu_dmp_grad.py is max(4 yard, 1e-6) with yard = err(float32 model, float64 model) <= 2.5e-5: the
    small cases' yards, here without a GPU (the hub's is computed there, once per module)."""
    from baseline_cases import rel
    for name in ("er300_T2", "er300_T3", "er300_T8", "er34", "isolated", "nnz0"):
        for start in ("mixed", "seeds"):
            lo, hi = M.model(name, start, "float32"), M.model(name, start, "float64")
            yards = [rel(a, b) for a, b in zip(lo[1:], hi[1:]) if b.size]
            print(f"{name}/{start}: yard " + " / ".join(f"{y:.1e}" for y in yards))
            assert max(yards) <= 2.5e-5
