"""Recorder of tests/golden/dmp_schedule_parent.json: the shape and the SHA-256 of the float32 bytes of what the scheduled DMP
marginals and their reverse sweep of the library of commit 8bd479b returned on an MI355X -- gnode_dmp_batch_schedule_f32 and
gnode_dmp_batch_schedule_backward_f32, when each had kernels and a host side of its own -- and with every call the workspace the
library asked for (`workspace_bytes`) and whether the one-workgroup form served its graph (`one_workgroup`).  The two GPU test
modules state the cases (each one's `parent_entries`) and recompute every entry, so the one statement of the batch kernels that
serves the constant and the scheduled entries now (csrc/gnode_dmp_batch.h) is held to those bits and sizes where the phases differ.

It ran from the repository's root with that commit's libgnode_hip.so (LIB: the path of the library to load; default: the
package's); run later it writes what the library of the day returns, which is the same file as long as those tests pass.

    forward/<case>/per_sample                       test_gpu_dmp_schedule.py's sched_out: B = 3, three phases, per-sample weights
                                                    and phase-0 gammas; hub is the general form, the others one workgroup
    forward/<case>/shared                           w_zero and hub: one matrix, two gamma tables alternating, both strides 0
    backward/<graph>/<per_sample|shared|P4>         the three gradients on the graphs on each side of the LDS boundary, B = 2,
                                                    T = 6; P4: a fourth phase that no step names (exact zeros)
    backward/er300_T2/P2, backward/nnz0/P3          no edge pass; no edge (the weights' gradient is null)

Every output is finite and not all zeros, and the block of a phase that no step names is exact zeros: asserted before hashing
(baseline_cases.schedule_entry, the modules' parent_entries).  Each direction holds an entry of each form
(baseline_cases.dmp_schedule_parent)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("gn-ode-sir_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

from gnode import _lib                                                                # noqa: E402

if os.environ.get("LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["LIB"])

import torch                                                                          # noqa: E402
import test_gpu_dmp_schedule as F                                                     # noqa: E402
import test_gpu_dmp_schedule_grad as R                                                # noqa: E402


def main():
    print("library", _lib.LIB_PATH, flush=True)
    dev, entries = torch.device("cuda:0"), {}
    for module in (F, R):
        for name, tables in module.PARENT_CASES:
            for key, entry in module.parent_entries(name, tables, dev):
                assert key not in entries, key
                entries[key] = entry
                print(key, entry["shape"], flush=True)
    for direction in ("forward/", "backward/"):
        assert {e["one_workgroup"] for k, e in entries.items() if k.startswith(direction)} == {True, False}, direction
    with open(os.path.join(ROOT, sys.argv[1] if len(sys.argv) > 1 else "tests/golden/dmp_schedule_parent.json"), "w") as f:
        json.dump({"parent": "8bd479b", "device": "MI355X", "entries": entries}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
