"""Drop-in for `DMP_SIR` of reference dmp.py:74-170 (the `model='dmp'` comparison column):
same constructor and `run(seed_list, maxTime)`, the message passing runs in libgnode_hip.so.

    DMP_SIR(weight_adj, nodes_gamma)        weight_adj: scipy sparse / dense [n, n] (the reference passes A*beta)
        .run(seed_list, maxTime) -> float32 tensor [maxTime, n, 3] = (Ps, Pi, Pr) on the GPU
                                                seed_list: seed ids, or an `InitialState` (an extension)
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from .graph import DeviceGraph


class DMP_SIR:
    def __init__(self, weight_adj, nodes_gamma, device="cuda"):
        A = sp.csr_matrix(weight_adj)
        A.sort_indices()
        self.N = A.shape[0]
        self.E = int(A.nnz)
        self.graph = DeviceGraph(A.indptr.astype(np.int32), A.indices.astype(np.int32))
        self.weights = torch.from_numpy(np.ascontiguousarray(A.data, dtype=np.float32)).to(device)
        self.nodes_gamma = torch.as_tensor(np.asarray(nodes_gamma, dtype=np.float32)).to(device)
        if self.nodes_gamma.numel() != self.N:
            raise _lib.GnodeError(f"DMP_SIR: nodes_gamma has {self.nodes_gamma.numel()} entries for {self.N} nodes")
        self.marginals = None

    def run(self, seed_list, maxTime):
        """seed_list: the seed ids, or (extension) a `gnode.ode_nn.InitialState`: Ps_0, Pi_0, Pr_0 are then its columns and
        the messages start from Phi_0 = Pi_0[src] (gnode_dmp_init_f32)."""
        from .ode_nn import InitialState
        if isinstance(seed_list, InitialState) and seed_list.n != self.N:
            raise ValueError(f"InitialState of {seed_list.n} nodes given for a graph of {self.N}")
        lib = _lib.load()
        out = torch.empty((int(maxTime), self.N, 3), dtype=torch.float32, device=self.weights.device)
        if isinstance(seed_list, InitialState):
            init = torch.from_numpy(seed_list.p.astype(np.float32)).to(out.device)
            ws = torch.empty(lib.gnode_dmp_init_workspace_bytes(self.graph.handle), dtype=torch.uint8, device=out.device)
            _lib.check(lib.gnode_dmp_init_f32(self.graph.handle, _lib.ptr(self.weights), _lib.ptr(self.nodes_gamma), _lib.ptr(init),
                                              int(maxTime), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
            self.marginals = out
            return out
        seeds = np.ascontiguousarray(list(seed_list), dtype=np.int32)
        ws = torch.empty(lib.gnode_dmp_workspace_bytes(self.graph.handle), dtype=torch.uint8, device=out.device)
        _lib.check(lib.gnode_dmp_f32(self.graph.handle, _lib.ptr(self.weights), _lib.ptr(self.nodes_gamma), _lib.host_ptr(seeds),
                                     int(seeds.shape[0]), int(maxTime), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                     _lib.stream_ptr()))
        self.marginals = out
        return out

    def output(self):
        return self.marginals
