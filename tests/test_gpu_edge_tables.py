"""GPU: the entries that read the handle's edge tables (src, rev: csrc/gnode_graph_plan.h) return the bits they returned when
every call built those tables on the device.  tests/golden/dmp_parent.json holds the DMP forward to that; this module holds
what it leaves open to tests/golden/edge_tables_parent.json, recorded from the library of commit 2dc701e on an MI355X by
tests/golden/make_golden_edge_tables_parent.py (which calls `record` below, so the inputs are stated once):

    dmp_batch_backward/<graph>   grad_w, grad_gamma, grad_init of gnode_dmp_batch_backward_f32, B = 2, T = 8, and its workspace
                                 size: karate (the one-workgroup form) and the two graphs of tests/test_gpu_dmp_grad.py on
                                 either side of the LDS boundary
    dmp_backward/karate          the same gradients of sample 0 from gnode_dmp_backward_f32 (the general form), its workspace size
    meanfield_rates/<graph>      outI, outS, outR and the step count of gnode_meanfield_rates_f64 with `w` given, B = 2, four
                                 output times, on karate and er150
    meanfield/karate             gnode_meanfield_f64: the scalar path

All of it is deterministic: the DMP sweep has no atomics, the mean-field's sums are sequential per thread and its error norm is
a maximum."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import dmp_grad_model as M
import test_gpu_dmp_grad as DG
import test_gpu_meanfield_rates as MF
from baseline_cases import f32_digest, gammas, weights
from meanfield_rates_model import golden_case, one_hot
from sir_cases import dev  # noqa: F401

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_tables_parent.json")
B, T = 2, 8
T_OUT = (0.0, 1.0, 2.5, 4.0)


def _graph(name):
    d = golden_case(name)
    return np.asarray(d["rowptr"], np.int32), np.asarray(d["col"], np.int32)


def _f64_digest(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float64 and np.isfinite(a).all()
    return hashlib.sha256(a.astype("<f8").tobytes()).hexdigest()


def _grads(key, got, **extra):
    assert all(np.isfinite(g).all() and g.any() for g in got), key
    return {key: {"shape": [list(g.shape) for g in got], "sha256": [f32_digest(g) for g in got], **extra}}


def _dmp(name, rp, ci, dev):
    e = DG.Entry(rp, ci, dev)
    n = e.n
    w, gam = np.stack([DG._w(rp, ci, 80 + b) for b in range(B)]), np.stack([gammas(n, 90 + b) for b in range(B)])
    init = np.stack([M.mixed_state(n, 95), M.seed_state(n, [1, n - 2])])
    G = M.grad_out_of(T, n, B)
    out = e.forward(w, gam, init, T)
    res = _grads(f"dmp_batch_backward/{name}", e.backward(w, gam, init, T, out, G), workspace_bytes=e.need(B, T),
                 one_workgroup=e.lds_bytes() <= DG.LDS_WORKGROUP)
    if name == "karate":
        res.update(_grads("dmp_backward/karate", e.solo(w[0], gam[0], init[0], T, out[0], e.up(G[0])),
                          workspace_bytes=int(e.lib.gnode_dmp_backward_workspace_bytes(e.g.handle, T))))
    return res


def _meanfield_rates(name, dev):
    rp, ci = _graph(name)
    n, rng = len(rp) - 1, np.random.default_rng(11)
    init = np.stack([one_hot(n, [0, n // 2]), rng.dirichlet([4, .5, .5], n)])
    beta, gam = rng.uniform(0.05, 0.3, (B, n)), rng.uniform(0.05, 0.4, (B, n))
    w = weights(len(ci), 0.2, 1.0, 12).astype(np.float64)                      # per directed entry: w_uv != w_vu
    status, out, steps = MF._rates_entry(dev, rp, ci, init, beta, w, gam, T_OUT)
    assert status == 0 and steps > 0
    return {f"meanfield_rates/{name}": {"shape": list(out[0].shape), "sha256": [_f64_digest(o) for o in out], "steps": steps}}


def _meanfield_scalar(dev):
    rp, ci = _graph("karate")
    out, steps = MF._scalar_entry(dev, rp, ci, [0, 33], 0.15, gammas(len(rp) - 1, 13).astype(np.float64), T_OUT)
    return {"meanfield/karate": {"shape": list(out[0].shape), "sha256": [_f64_digest(o) for o in out], "steps": steps}}


CASES = {"dmp/karate": lambda dev: _dmp("karate", *_graph("karate"), dev),
         "dmp/last_fit": lambda dev: _dmp("last_fit", *DG.form_graphs()["last_fit"], dev),
         "dmp/first_unfit": lambda dev: _dmp("first_unfit", *DG.form_graphs()["first_unfit"], dev),
         "meanfield_rates/karate": lambda dev: _meanfield_rates("karate", dev),
         "meanfield_rates/er150": lambda dev: _meanfield_rates("er150", dev),
         "meanfield/karate": _meanfield_scalar}


def record(dev):
    """{key: entry} of every case: what the fixture holds"""
    out = {}
    for make in CASES.values():
        out.update(make(dev))
    return out


@functools.lru_cache(maxsize=None)
def parent():
    with open(FIXTURE) as f:
        return json.load(f)["entries"]


def test_fixture_takes_both_forms():
    p = parent()
    assert len(p) == 7
    assert p["dmp_batch_backward/karate"]["one_workgroup"] and p["dmp_batch_backward/last_fit"]["one_workgroup"]
    assert not p["dmp_batch_backward/first_unfit"]["one_workgroup"]
    assert all(e["steps"] > 0 for k, e in p.items() if k.startswith("meanfield"))


@pytest.mark.parametrize("case", list(CASES))
def test_bits_are_the_parents(case, dev):
    got = CASES[case](dev)
    for key, entry in got.items():
        assert entry == parent()[key], key
