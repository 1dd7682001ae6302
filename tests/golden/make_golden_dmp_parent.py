"""Recorder of tests/golden/dmp_parent.json: the shape and the SHA-256 of the float32 bytes of every DMP output that the library
of commit 893d874 returned on an MI355X, when gnode_dmp_f32 and gnode_dmp_init_f32 still had kernels of their own
(k_dmp_out0 / _init / _node / _edge<INIT>).  tests/test_gpu_baselines.py and tests/test_gpu_dmp_batch.py recompute every
entry and compare digests, so the one statement of the recurrence that serves all three entries now is held to those bits.

It ran from the repository's root with that commit's libgnode_hip.so; run later it writes what the library of the day returns,
which is the same file as long as those tests pass.  The inputs are the tests' own (this script imports their helpers):

    dmp_f32/<case>                  DMP_SIR.run(seeds, T) for the ten DMP_CASES; `workspace_bytes` is gnode_dmp_workspace_bytes
    dmp_init_f32/<case>/<b>         the solo runs of test_batch_sample_is_its_solo_run: 8 cases, 3 samples each
    dmp_batch/<case>                their batches of 3; `batch_workspace_bytes` is gnode_dmp_batch_workspace_bytes(B)
    dmp_init_f32/form/<tag>/<b>     the solo runs of test_each_form_and_boundary_is_the_solo_run: 4 graphs, 2 samples each
    dmp_batch/form/<tag>            their batches of 2

Every output is finite (w_one at its T = 3 included): asserted before hashing."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("gn-ode-sir_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import test_gpu_dmp_batch as B                                                        # noqa: E402
from baseline_cases import DMP_CASES, dmp_model, f32_digest                           # noqa: E402
from gnode import _lib                                                                # noqa: E402

ENTRIES = []


def rec(key, out, **extra):
    a = out.cpu().numpy()
    assert a.dtype == np.float32 and np.isfinite(a).all(), key
    ENTRIES.append({"key": key, "shape": list(a.shape), "sha256": f32_digest(a), **extra})
    print(key, a.shape, flush=True)


def main():
    lib = _lib.load()
    for name, make in DMP_CASES.items():
        c = make()
        m = dmp_model(c)
        need = int(lib.gnode_dmp_workspace_bytes(m.graph.handle))
        assert need == int(lib.gnode_dmp_init_workspace_bytes(m.graph.handle))
        rec(f"dmp_f32/{name}", m.run(c["seeds"], c["T"]), workspace_bytes=need)
    for name in B.CASES:
        c, M, ps, gam = B.batch_case(name)
        for b in range(3):
            rec(f"dmp_init_f32/{name}/{b}", B._solo(M * B.SCALE[b], gam[b], B._state(ps[b]), c["T"]))
        rec(f"dmp_batch/{name}", B.batch_out(name), batch_workspace_bytes=B._batch_need(M, 3))
    for tag in B.FORM_TAGS:
        inputs, got = B.form_out(tag)
        for b in range(2):
            rec(f"dmp_init_f32/form/{tag}/{b}", B.form_solo(inputs, b))
        rec(f"dmp_batch/form/{tag}", got, batch_workspace_bytes=B._batch_need(inputs[0], 2))
    assert len({e["key"] for e in ENTRIES}) == len(ENTRIES) == 10 + 8 * 4 + 4 * 3
    with open(os.path.join(ROOT, sys.argv[1] if len(sys.argv) > 1 else "tests/golden/dmp_parent.json"), "w") as f:
        json.dump({"parent": "893d874", "device": "MI355X", "entries": ENTRIES}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
