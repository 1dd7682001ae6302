"""Recorder of tests/golden/dmp_candidates_parent.json: the shape and the SHA-256 of the float64 bytes of every table that the four
candidate sweeps of the library of commit 40c1952 returned on an MI355X -- gnode_dmp_source_scores_f32,
gnode_dmp_source_batch_scores_f32, gnode_dmp_source_events_scores_f32 and gnode_dmp_outbreak_sizes_f32, when each had kernels, a
workspace and a host side of its own -- and with every table what the library answered for its call and graph: the workspace
(`workspace_bytes`), the LDS of the one-workgroup form (`lds_bytes`) and, for the batch and events entries, the `tile`.  The four
GPU test modules state the cases (each one's `parent_entries`) and recompute every entry, so the one statement of the sweep that
serves all four entries now (csrc/gnode_dmp_sweep.h) is held to those bits and sizes.

It ran from the repository's root with that commit's libgnode_hip.so (LIB: the path of the library to load; default: the
package's); run later it writes what the library of the day returns, which is the same file as long as those tests pass.

    source/<case>/T<T>                              cand_list's five candidates on mixed_obs: er34, isolated, nnz0 (one
                                                    workgroup), hub, big_er (general; big_er has two blocks per candidate)
    source_batch/<case>/T<T>/O<O>                   the same cases, O in {1, W - 1, W, W + 1, 2 W + 1} for the tile W; and `edge`,
                                                    the graph at the LDS edge, where the tile narrows
    source_events/<case>/T<T>/R<R>/floor<floor>     karate, strided, general and `edge`; rows of all six codes
    outbreak/<case>/T<T>/<action>/<valued|null>     the source cases, both actions on the mixed start, the last candidate -1

Every output is finite: asserted before hashing (baseline_cases.candidates_entry)."""
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
import test_gpu_dmp_outbreak as K                                                     # noqa: E402
import test_gpu_dmp_source as S                                                       # noqa: E402
import test_gpu_dmp_source_batch as B                                                 # noqa: E402
import test_gpu_dmp_source_events as E                                                # noqa: E402


def main():
    print("library", _lib.LIB_PATH, flush=True)
    dev, entries = torch.device("cuda:0"), {}
    for module in (S, B, E, K):
        for name, T in module.PARENT_CASES:
            for key, entry in module.parent_entries(name, T, dev):
                assert key not in entries, key
                entries[key] = entry
                print(key, entry["shape"], flush=True)
    with open(os.path.join(ROOT, sys.argv[1] if len(sys.argv) > 1 else "tests/golden/dmp_candidates_parent.json"), "w") as f:
        json.dump({"parent": "40c1952", "device": "MI355X", "entries": entries}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
