"""CPU: the one model of tests/sir_model.py and the cases of tests/sir_cases.py are held to the oracle (`sir_philox`, `dmp_sir`),
and -- `test_model_reproduces_the_parent_models` -- to a digest of every array that the four models it replaced
(per-node, per-edge, per-trajectory, drawn start) returned at every call under tests/ at commit 35424da, recorded by
tests/golden/make_golden_sir_model.py.  The GPU modules take their expected arrays from the same `sir_cases.expected`, so a
green digest test means that they compare with the values they compared with before.  The closed forms (the one-way path,
the tree's marginals, one-hot rows that ignore the coin) are in tests/test_sir_edges_model.py and tests/test_sir_init_model.py.

The four earlier test files also compared one model with another: per-edge against per-node at w = beta[col], events against
the per-node counts, the one-hot start against the per-edge model.  With one model those are tautologies; the digest test,
in which the digests of both recorded sides have to be met by the same arrays, replaces them."""
import hashlib
import json
import os

import numpy as np
import pytest

import gnode_oracle as O
import sir_cases
import sir_model as M
from sir_cases import CONST, EVENTS, RS

def _get(key):
    return sir_cases.case(key), sir_cases.expected(key)


# ------------------------------------------------------------------------------------------- the gate: the parent's outputs
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sir_model_parent.json")) as _f:
    PARENT = {e["key"]: e for e in json.load(_f)["entries"]}


def _digest(a):
    return hashlib.sha256(f"{a.dtype}{a.shape}".encode() + np.ascontiguousarray(a).tobytes()).hexdigest()


def test_every_case_is_recorded():
    assert {e["case"] for e in PARENT.values()} == set(sir_cases.CASES)


@pytest.mark.parametrize("key", sorted(PARENT))
def test_model_reproduces_the_parent_models(key):
    """Every array an earlier model returned at this call site, by digest; the recorded scalars of the recipe; and the
    liveness checks of the case, on the model's output alone."""
    entry = PARENT[key]
    c, want = _get(entry["case"])
    for name in ("T", "rng_seed", "sim_offset"):
        assert entry["args"][name] == getattr(c, name), name
    for name, sha in entry["sha256"].items():
        if name == "singles":               # the parent's one-trajectory calls, stacked: each row of this run on its own
            got = np.stack([M.counts(want.t_inf[j:j + 1], want.t_rec[j:j + 1], c.T, hold_row0=True) for j in range(c.sims)])
        else:
            assert entry["args"]["sims"] == c.sims
            got = getattr(want, name)
        assert _digest(got) == sha, f"{key}: {name} is not what {entry['fn']} returned at the parent commit"
    for check in c.live:
        check(c, want)


# ------------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("i", range(len(CONST)))
def test_constant_rates_equal_scalar_oracle(i):
    """One constant as a scalar, per node and per CSR position, with gamma as a scalar and per node: `sir_philox`'s counts."""
    c, _ = _get(f"cpu/const/{i}")
    graph, seeds, beta, gamma, sims, T, off = CONST[i]
    want = O.sir_philox(c.n, c.rp, c.ci, seeds, beta, gamma, sims, T, rng_seed=RS, sim_offset=off)
    assert want[2, -1].sum() > 0 or gamma == 0.0
    forms = (dict(beta=beta), dict(beta=np.full(c.n, beta)), dict(w=np.full(len(c.ci), beta)))
    for rate in forms:
        for g in (gamma, np.full(c.n, gamma)):
            ev = M.sir_events(c.n, c.rp, c.ci, seeds, M.infection_thresholds(c.n, c.ci, **rate), g, sims, T, RS, off)
            assert np.array_equal(M.counts(*ev, T, hold_row0=True), want), (list(rate), np.ndim(g))


def test_edge_rates_behave():
    """beta_v = 0 nodes never leave S, gamma_u = 1 nodes are in I for exactly one step, gamma_u = 0 nodes never reach R,
    and every trajectory has every node in exactly one compartment."""
    case, want = _get("cpu/behave")
    b0, g1, g0, sims = case.sets["b0"], case.sets["g1"], case.sets["g0"], case.sims
    c = want.counts.astype(np.int64)
    assert np.all(c[0, 1:] + c[1, 1:] + c[2, 1:] == sims)
    assert np.all(c[0, 1:, b0] == sims)                                   # shielded: susceptible for ever
    ever = sims - c[0, -1]                                                # trajectories in which the node was infected
    assert ever[g1].sum() > 0 and ever[g0].sum() > 0                      # (the epidemic did reach such nodes)
    # gamma = 1: a node infected at step t is in I at t and in R from t + 1 on, so over all steps its I count sums to
    # one per infection that happened before the last step
    inf_before_last = sims - c[0, -2]
    assert np.array_equal(c[1, 1:-1].sum(0)[g1], inf_before_last[g1])
    assert np.array_equal(c[2, -1][g1], inf_before_last[g1])
    assert not c[2][:, g0].any()                                          # gamma = 0: never recovered
    assert np.array_equal(c[1, -1][g0], ever[g0])                         # ... still infected at the end


@pytest.mark.parametrize("graph", ["karate", "er200"])
def test_per_node_rate_is_the_targets_not_the_sources(graph):
    """beta per node is looked up at the column of the entry: the same rates indexed by the row give other counts."""
    want = _get(f"cpu/target/{graph}")[1].counts
    assert want[2, -1].sum() > 0
    assert not np.array_equal(_get(f"cpu/target-src/{graph}")[1].counts, want)


@pytest.mark.parametrize("name", list(EVENTS))
@pytest.mark.parametrize("rates", ["scalar", "arrays"])
def test_events_and_curves_equal_oracle(name, rates):
    """The events, folded, are the counts of `sir_philox`, each curve is the node sum of the oracle's single-trajectory
    call (scalar rates; for arrays the digest test holds both to the parent's per-node model), and recovery never falls in
    the step of infection."""
    c, got = _get(f"cpu/events/{name}/{rates}")
    n, sims, T, off = c.n, c.sims, c.T, c.sim_offset
    t_inf, t_rec, curves = got.t_inf, got.t_rec, got.curves
    assert t_inf.dtype == np.int16 and t_inf.shape == (sims, n) and curves.shape == (sims, T, 3)
    assert got.counts[2, -1].sum() > 0 and (t_inf == -1).any()
    k = len(set(c.start))
    if rates == "scalar":
        assert np.array_equal(got.counts, O.sir_philox(n, c.rp, c.ci, c.start, c.beta, c.gamma, sims, T, c.rng_seed, sim_offset=off))
    for j in range(sims):
        if rates == "scalar":
            one = O.sir_philox(n, c.rp, c.ci, c.start, c.beta, c.gamma, 1, T, c.rng_seed, sim_offset=off + j).astype(np.int64)
            node_sums = one.sum(axis=2).T                  # [T, 3]; with sims = 1 the row-0 quirk IS the initial state
            assert np.array_equal(curves[j].astype(np.int64), node_sums), (name, j)
        assert tuple(curves[j, 0]) == (n - k, k, 0)
    both = (t_inf >= 0) & (t_rec >= 0)
    assert both.any() and np.all(t_rec[both] > t_inf[both])
    assert np.all(t_inf[t_rec >= 0] >= 0)                  # nobody recovers without having been infected
    assert np.all(curves.astype(np.int64).sum(axis=2) == n)


# --------------------------------------------------------------------------------------------------------- drawn starts
def test_one_hot_start_is_the_seed_list_call():
    """Rows t >= 1 and the events of the seed-list call, and `sims` times its row 0: against `sir_philox` (scalar rates) and
    against the seed-list start of the model itself (per-edge weights)."""
    c, got = _get("cpu/onehot/scalar")
    want = O.sir_philox(c.n, c.rp, c.ci, c.seeds, 0.3, 0.2, c.sims, c.T, rng_seed=17, sim_offset=3)
    assert want[1, 1:].any() and want[2, 1:].any()
    assert np.array_equal(got.counts[:, 1:], want[:, 1:]) and np.array_equal(got.counts[:, 0], c.sims * want[:, 0])
    (c, got), (_, want) = _get("cpu/onehot/p"), _get("cpu/onehot/seeds")
    assert np.array_equal(got.counts[:, 1:], want.counts[:, 1:]) and np.array_equal(got.counts[:, 0], c.sims * want.counts[:, 0])
    assert np.array_equal(got.t_inf, want.t_inf) and np.array_equal(got.t_rec, want.t_rec)
