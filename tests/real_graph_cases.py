"""Inputs of the real-graph fixtures (tests/golden/real_*.npz, written by tests/golden/make_golden_realgraphs.py), rebuilt
from the seeds they store: shared by the CPU check of the oracle (test_real_graphs_golden.py) and the GPU check of the
product (test_gpu_real_graphs.py), so both hold the same inputs to the same float64 numbers."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
MULTI = ["real_multi_4-2-3-1-0-4-2-3_H8_T20", "real_multi_4-4-4-4-4-4-4-4_H8_T20"]     # compositions A and B
SINGLE = ["real_single_fbsocial_H64_T30", "real_single_wikivote_H64_T30"]
WIKI = 4                                                                             # index of wiki-vote in real_graphs.npz

_synth_mod = None


def synth():
    """gnode/synth.py on its own (numpy only: importing the gnode package would load the HIP library)"""
    global _synth_mod
    if _synth_mod is None:
        spec = importlib.util.spec_from_file_location("_synth_real", os.path.join(os.path.dirname(HERE), "gn-ode-sir_amd", "gnode", "synth.py"))
        _synth_mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_synth_mod)
    return _synth_mod


def graphs():
    """[(rowptr, col)] of dolphins, fb-food, fb-social, openflights, wiki-vote (largest components, create_graphs' order)."""
    d = np.load(os.path.join(GOLDEN, "real_graphs.npz"))
    return [(d[f"indptr{j}"], d[f"indices{j}"]) for j in range(len(d["names"]))]


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def inputs(d, gs):
    """(x, P, y) of a fixture: multi -> x [sumN, 3+H], y [sumN, T, 3]; single -> x [1, n, 3+H], y [n, T, 3]."""
    from golden.labels import closed_form_labels
    sy = synth()
    H, maxTime = int(d["H"]), int(d["maxTime"])
    P = sy.linear_params(H, seed=int(d["param_seed"]))
    if "picks" in d:
        xs = []
        for j, p in enumerate(d["picks"]):
            xi = sy.samples(gs[p][0].shape[0] - 1, 1, H, seed=int(d["sample_seed"]) + j)[0]
            xi[0, 3 + 2] = p + 1                                                   # the graph marker, ode_nn_ngraphs.py:333
            xs.append(xi)
        x = np.concatenate(xs, 0)
        x[:, 3] *= np.float32(d["beta_scale"])
    else:
        n = gs[int(d["graph"])][0].shape[0] - 1
        x = sy.samples(n, 1, H, seed=int(d["sample_seed"]))
        x[..., 3] *= np.float32(d["beta_scale"])
    rows = x.shape[0] if x.ndim == 2 else x.shape[1]
    y = closed_form_labels(1, rows, maxTime).reshape(rows, maxTime, 3)
    return x, P, y
