#!/usr/bin/env python3
"""Golden vectors for the mean-field with per-node and per-contact rates: the reference's own `runge_kutta_order4(sir, A,
...)` (ode_nn.py:214-233) executed unchanged -- it is numpy broadcasting, so a weighted dense A and array rates go through
it as they are.  A is the dense TRANSPOSE of the weight matrix, A[v, u] = M[u, v] = the rate at which u infects v, since
`sir` forms A @ I for the target's row.  LSODA runs at its default tolerances.  Import shims as in make_golden.py; no
pickle of the reference is loaded.

    karate  per-contact weights in [0.02, 0.15], a fifth of the edges one-way (the reverse entry zeroed), per-node gamma in
            [0.1, 0.5], beta = 1, seeds [0, 33], deltaT 1, maxTime 20
    er150   gnm_random_graph(150, 700, seed=11), per-node beta in [0.02, 0.1], gamma 0.4, seed [3], deltaT 0.5, maxTime 15
"""
import os
import sys

import numpy as np
import networkx as nx
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402


def _csr(G):
    A = sp.csr_matrix(nx.adjacency_matrix(G, nodelist=sorted(G.nodes())), dtype=np.float64)
    A.data[:] = 1.0
    A.sort_indices()
    return A


def _karate():
    A = _csr(nx.karate_club_graph())
    n, rng = A.shape[0], np.random.default_rng(41)
    w = rng.uniform(0.02, 0.15, size=A.nnz)
    src = np.repeat(np.arange(n), np.diff(A.indptr))
    und = np.flatnonzero(src < A.indices)                           # one position per undirected edge: u -> v with u < v
    one_way = rng.choice(und, size=len(und) // 5, replace=False)    # u -> v stays, v -> u never transmits
    M = sp.csr_matrix((w, A.indices, A.indptr), shape=(n, n)).tolil()
    for p in one_way:
        M[A.indices[p], src[p]] = 0.0
    M = sp.csr_matrix(M)
    M.sort_indices()
    w = np.zeros(A.nnz)
    for u in range(n):                                              # back into A's positions: the zeros stay stored
        for p in range(A.indptr[u], A.indptr[u + 1]):
            w[p] = M[u, A.indices[p]]
    return dict(A=A, w=w, beta=None, gamma=rng.uniform(0.1, 0.5, size=n), seeds=[0, 33], deltaT=1, maxTime=20)


def _er150():
    A = _csr(nx.gnm_random_graph(150, 700, seed=11))
    rng = np.random.default_rng(42)
    return dict(A=A, w=None, beta=rng.uniform(0.02, 0.1, size=150), gamma=0.4, seeds=[3], deltaT=0.5, maxTime=15)


def main():
    MG._install_import_shims()
    sys.path.insert(0, "/root/reference")
    import ode_nn as REF
    for name, c in (("karate", _karate()), ("er150", _er150())):
        A, n = c["A"], c["A"].shape[0]
        M = A.toarray() if c["w"] is None else sp.csr_matrix((c["w"], A.indices, A.indptr), shape=(n, n)).toarray()
        dense = np.ascontiguousarray(M.T)                           # A[v, u] = M[u, v]
        beta = 1.0 if c["beta"] is None else c["beta"]
        gamma = c["gamma"] if np.ndim(c["gamma"]) else c["gamma"] * np.ones(n)
        I_t, S_t, R_t = REF.runge_kutta_order4(REF.sir, dense, n, list(c["seeds"]), beta, gamma, c["deltaT"], c["maxTime"])
        none = np.zeros(0)
        np.savez_compressed(os.path.join(HERE, f"meanfield_rates_{name}.npz"), rowptr=A.indptr.astype(np.int32),
                            col=A.indices.astype(np.int32), seeds=np.asarray(c["seeds"], np.int32),
                            beta=none if c["beta"] is None else c["beta"], w=none if c["w"] is None else c["w"],
                            gamma=np.asarray(gamma, np.float64), deltaT=np.float64(c["deltaT"]), maxTime=np.int32(c["maxTime"]),
                            I=np.asarray(I_t), S=np.asarray(S_t), R=np.asarray(R_t))
        print(name, np.asarray(I_t).shape, "zero weights:", 0 if c["w"] is None else int((c["w"] == 0).sum()),
              "mean R at the end:", float(np.asarray(R_t)[-1].mean()))


if __name__ == "__main__":
    main()
