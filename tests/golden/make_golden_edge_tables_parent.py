"""Recorder of tests/golden/edge_tables_parent.json: the shapes and the SHA-256 of the bytes of the DMP gradients and the
mean-field outputs that the library of commit 2dc701e returned on an MI355X, when every DMP and weighted mean-field call still
built the source / reverse-edge tables on the device (k_dmp_setup, k_mf_w_in's search) and the scalar mean-field had a kernel
of its own (k_mf_rhs).  tests/test_gpu_edge_tables.py states the cases (its docstring lists the keys) and recomputes every entry.

It ran from the repository's root with that commit's libgnode_hip.so (LIB: the path of the library to load; default: the
package's); run later it writes what the library of the day returns, which is the same file as long as that test passes."""
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
import test_gpu_edge_tables as E                                                      # noqa: E402


def main():
    print("library", _lib.LIB_PATH, flush=True)
    entries = E.record(torch.device("cuda:0"))
    assert len(entries) == 7
    for k, v in entries.items():
        print(k, v["shape"], flush=True)
    with open(os.path.join(ROOT, sys.argv[1] if len(sys.argv) > 1 else "tests/golden/edge_tables_parent.json"), "w") as f:
        json.dump({"parent": "2dc701e", "device": "MI355X", "entries": entries}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
