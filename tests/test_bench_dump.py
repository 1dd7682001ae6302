"""bench.py --dump-outputs, host side: the per-chunk (S, I, R) the timed path returns land in DIR/{S,I,R}.npy as float32
[grid points, samples, nodes], whole or as the fixed seeded node sample, under the 64 MB budget."""
import os

import numpy as np
import pytest

import bench


@pytest.mark.parametrize("n,n_out,B,chunk", [(50, 7, 3, 2), (75000, 60, 8, 8), (75000, 60, 8, 3)])
def test_dump_outputs_layout_and_budget(tmp_path, n, n_out, B, chunk):
    torch = pytest.importorskip("torch")
    full = np.random.default_rng(1).random((n_out, B, n), dtype=np.float32)
    outs = []
    for b0 in range(0, B, chunk):
        s = torch.from_numpy(np.ascontiguousarray(full[:, b0:b0 + chunk].reshape(n_out, -1)))   # rows: sample-major, as ops.forward
        outs.append((s, s + 1, s + 2))
    info = bench.dump_outputs(outs, str(tmp_path), n)
    S, I, R = (np.load(tmp_path / f"{c}.npy") for c in "SIR")
    k = S.shape[2]
    nodes = np.arange(n) if k == n else np.sort(np.random.default_rng(0).choice(n, size=k, replace=False))
    assert (k == n) == (info["nodes"] == "all")
    for got, off in ((S, 0), (I, 1), (R, 2)):
        assert got.dtype == np.float32 and got.shape == (n_out, B, k)
        assert np.array_equal(got, full[:, :, nodes] + off)
    assert sum(os.path.getsize(tmp_path / f"{c}.npy") for c in "SIR") <= bench.DUMP_BUDGET_BYTES
    again = tmp_path / "again"
    bench.dump_outputs(outs, str(again), n)
    assert all(np.array_equal(np.load(again / f"{c}.npy"), a) for c, a in zip("SIR", (S, I, R)))
