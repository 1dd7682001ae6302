"""ctypes binding of libgnode_hip.so (the C ABI declared in include/gnode.h).

There is no CPU fallback: if the HIP library is missing or a tensor is not on a
GPU the calls raise.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgnode_hip.so")


class GnodeError(RuntimeError):
    pass


class Params(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "odefunc_linear_weight", "odefunc_linear_bias", "linearS1_weight", "linearS1_bias",
        "linear3_weight", "linear3_bias", "linearS2_weight", "linearS2_bias")]


class Grads(C.Structure):
    _fields_ = Params._fields_


_vp, _i32, _i64, _sz, _f64, _int, _u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_double, C.c_int, C.c_uint64
_P, _pi32, _pi64, _pf64 = C.POINTER(Params), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
_BWD = [_vp, _vp, _P, _vp, _i32, _vp, _i32, _vp, _vp, _sz, _vp, _vp, _vp, _P, _i64, _i32, _vp, _sz, _vp, _i32, _i32]
_BWD_RK4 = [_vp, _vp, _P, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _P, _i64, _i32, _vp, _sz, _vp]
_SIR = [_vp, _vp, _i32, _f64, _f64, _i64, _i64, _i32, _u64, _vp, _vp, _sz, _vp]
_L1 = [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _vp]

# The C ABI of include/gnode.h, once: name -> (restype, argtypes).  `load` applies it; tests/test_abi.py holds it against the
# header's prototypes.  (The _dx / _scan / _counted entries take their base entry's arguments, the extra one last.)
ABI = {
    "gnode_last_error": (C.c_char_p, []),
    "gnode_version": (_int, []),
    "gnode_graph_create": (_int, [_vp, _vp, _i32, _i64, C.POINTER(_vp)]),
    "gnode_graph_destroy": (_int, [_vp]),
    "gnode_graph_info": (_int, [_vp, _pi32, _pi64, _pi32]),
    "gnode_rhs_workspace_bytes": (_sz, [_vp, _i64, _i32]),
    "gnode_rhs_f32": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _sz, _vp]),
    "gnode_forward_workspace_bytes": (_sz, [_vp, _i64, _i32, _i32]),
    "gnode_forward_f32": (_int, [_vp, _vp, _P, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _i64, _i32, _vp, _sz,
                                 _vp, _i32, _pi32]),
    "gnode_forward_status": (_int, [_i64, _i32, _i32, _vp, _vp, _pi32]),
    "gnode_backward_status": (_int, [_i64, _i32, _vp, _vp, _pi32]),
    "gnode_forward_path": (_int, [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _pi32]),
    "gnode_sol_carries_neighbour_sums": (_int, [_vp, _i64, _i32, _i32, _i32, _i32]),
    "gnode_forward_keep_bytes": (_sz, [_vp, _i64, _i32, _i32, _i32]),
    "gnode_backward_workspace_bytes": (_sz, [_vp, _i64, _i32]),
    "gnode_backward_f32": (_int, _BWD),
    "gnode_backward_dx_f32": (_int, _BWD + [_vp]),
    "gnode_rhs_vjp_workspace_bytes": (_sz, [_vp, _i64, _i32]),
    "gnode_rhs_vjp_f32": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _sz, _vp]),
    "gnode_backward_rk4_workspace_bytes": (_sz, [_vp, _i64, _i32]),
    "gnode_backward_rk4_f32": (_int, _BWD_RK4),
    "gnode_backward_rk4_dx_f32": (_int, _BWD_RK4 + [_vp]),
    "gnode_backward_discrete_workspace_bytes": (_sz, [_vp, _i64, _i32]),
    "gnode_backward_discrete_f32": (_int, [_vp, _vp, _P, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _P, _vp, _i64, _i32,
                                           _vp, _sz, _vp]),
    "gnode_backward_discrete_keep_f32": (_int, _BWD + [_vp]),
    "gnode_backward_discrete_path": (_int, [_vp, _i64, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32]),
    "gnode_sir_workspace_bytes": (_sz, [_vp, _i32]),
    "gnode_sir_coins_workspace_bytes": (_sz, []),
    "gnode_sir_mc_philox": (_int, _SIR),
    "gnode_sir_mc_philox_scan": (_int, _SIR),
    "gnode_sir_mc_philox_counted": (_int, _SIR + [C.POINTER(_u64)]),
    "gnode_sir_nodes_workspace_bytes": (_sz, [_vp, _i32]),
    "gnode_sir_mc_philox_nodes": (_int, [_vp, _vp, _i32, _vp, _vp, _i64, _i64, _i32, _u64, _vp, _vp, _sz, _vp, _i32]),
    "gnode_sir_traj_workspace_bytes": (_sz, [_vp, _i32]),
    "gnode_sir_mc_philox_traj": (_int, [_vp, _vp, _i32, _f64, _f64, _vp, _vp, _i64, _i64, _i32, _u64, _vp, _vp, _vp, _vp, _sz, _vp, _i32]),
    "gnode_sir_edges_workspace_bytes": (_sz, [_vp, _i32]),
    "gnode_sir_mc_philox_edges": (_int, [_vp, _vp, _i32, _vp, _f64, _vp, _i64, _i64, _i32, _u64, _vp, _vp, _sz, _vp, _i32]),
    "gnode_sir_mc_philox_traj_edges": (_int, [_vp, _vp, _i32, _vp, _f64, _vp, _i64, _i64, _i32, _u64, _vp, _vp, _vp, _vp, _sz, _vp, _i32]),
    "gnode_sir_init_workspace_bytes": (_sz, [_vp, _i32]),
    "gnode_sir_mc_philox_init": (_int, [_vp, _vp, _f64, _vp, _vp, _f64, _vp, _i64, _i64, _i32, _u64, _vp, _vp, _vp, _vp, _sz, _vp, _i32]),
    "gnode_sir_schedule_workspace_bytes": (_sz, [_vp, _i32, _i32]),
    "gnode_sir_mc_philox_schedule": (_int, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i64, _i64, _i32, _u64, _vp, _vp, _vp, _vp, _sz, _vp, _i32]),
    "gnode_sir_sweep_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32, _i32]),
    "gnode_sir_mc_philox_sweep": (_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _i64, _i64, _i32, _u64, _vp, _vp, _vp, _sz,
                                         _vp, _i32]),
    "gnode_sir_sweep_scores_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32, _i32, _i32]),
    "gnode_sir_mc_philox_sweep_scores": (_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i64, _i64, _i32,
                                                _u64, _vp, _vp, _sz, _vp, _i32]),
    "gnode_sir_sweep_timed_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32, _i32, _i32, _i32]),
    "gnode_sir_mc_philox_sweep_timed": (_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i64,
                                               _i64, _i32, _u64, _vp, _vp, _sz, _vp, _i32]),
    "gnode_sir_sweep_posterior_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "gnode_sir_mc_philox_sweep_posterior": (_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp,
                                                   _i32, _i64, _i64, _i32, _u64, _vp, _vp, _vp, _sz, _vp, _i32]),
    "gnode_sir_mc_philox_sweep_posterior_strata": (_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32,
                                                          _vp, _i32, _i32, _i64, _i64, _i32, _u64, _vp, _vp, _vp, _sz, _vp, _i32]),
    "gnode_sir_mc_coins": (_int, [_vp, _vp, _i64, _i32, _vp, _i32, _f64, _f64, _i64, _i32, _vp, _i64, _vp, _pi64, _vp, _sz, _vp]),
    "gnode_dmp_workspace_bytes": (_sz, [_vp]),
    "gnode_dmp_f32": (_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _sz, _vp]),
    "gnode_dmp_init_workspace_bytes": (_sz, [_vp]),
    "gnode_dmp_init_f32": (_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _sz, _vp]),
    "gnode_dmp_batch_workspace_bytes": (_sz, [_vp, _i32]),
    "gnode_dmp_batch_lds_bytes": (_sz, [_vp]),
    "gnode_dmp_batch_f32": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i32, _i32, _vp, _vp, _sz, _vp]),
    "gnode_dmp_batch_schedule_workspace_bytes": (_sz, [_vp, _i32, _i32]),
    "gnode_dmp_batch_schedule_f32": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _sz, _vp]),
    "gnode_dmp_batch_backward_lds_bytes": (_sz, [_vp]),
    "gnode_dmp_batch_backward_workspace_bytes": (_sz, [_vp, _i32, _i32]),
    "gnode_dmp_batch_backward_f32": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gnode_dmp_batch_schedule_backward_workspace_bytes": (_sz, [_vp, _i32, _i32]),
    "gnode_dmp_batch_schedule_backward_f32": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                                     _vp]),
    "gnode_dmp_backward_workspace_bytes": (_sz, [_vp, _i32]),
    "gnode_dmp_backward_f32": (_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gnode_dmp_source_lds_bytes": (_sz, [_vp]),
    "gnode_dmp_source_workspace_bytes": (_sz, [_vp, _i32, _i32]),
    "gnode_dmp_source_scores_f32": (_int, [_vp, _vp, _vp, _vp, _i32, _vp, C.c_float, _i32, _vp, _vp, _sz, _vp]),
    "gnode_dmp_source_batch_tile": (_int, [_vp]),
    "gnode_dmp_source_batch_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32]),
    "gnode_dmp_source_batch_scores_f32": (_int, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, C.c_float, _i32, _vp, _i64, _vp, _sz, _vp]),
    "gnode_dmp_source_events_tile": (_int, [_vp]),
    "gnode_dmp_source_events_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32]),
    "gnode_dmp_source_events_scores_f32": (_int, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, C.c_float, _i32, _vp, _i64, _vp, _sz, _vp]),
    "gnode_dmp_outbreak_lds_bytes": (_sz, [_vp]),
    "gnode_dmp_outbreak_workspace_bytes": (_sz, [_vp, _i32, _i32]),
    "gnode_dmp_outbreak_sizes_f32": (_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _sz, _vp]),
    "gnode_dmp_source_events_schedule_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32, _i32]),
    "gnode_dmp_source_events_scores_schedule_f32": (_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _i32, C.c_float, _i32, _vp,
                                                           _i64, _vp, _sz, _vp]),
    "gnode_dmp_outbreak_schedule_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32]),
    "gnode_dmp_outbreak_sizes_schedule_f32": (_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _sz,
                                                     _vp]),
    "gnode_meanfield_workspace_bytes": (_sz, [_vp]),
    "gnode_meanfield_f64": (_int, [_vp, _vp, _i32, _f64, _vp, _vp, _i32, _f64, _f64, _vp, _vp, _vp, _pi64, _vp, _sz, _vp]),
    "gnode_meanfield_init_f64": (_int, [_vp, _vp, _f64, _vp, _vp, _i32, _f64, _f64, _vp, _vp, _vp, _pi64, _vp, _sz, _vp]),
    "gnode_meanfield_rates_workspace_bytes": (_sz, [_vp, _i32]),
    "gnode_meanfield_rates_f64": (_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _f64, _f64, _vp, _vp, _vp, _pi64, _vp, _sz, _vp]),
    "gnode_meanfield_rates_steps_f64": (_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _f64, _f64, _vp, _vp, _vp, _pi64, _vp, _sz, _vp,
                                               _vp, _i64, _pi64, _vp]),
    "gnode_meanfield_rates_backward_workspace_bytes": (_sz, [_vp, _i32, _i32]),
    "gnode_meanfield_rates_backward_f64": (_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                  _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gnode_l1_loss_workspace_bytes": (_sz, []),
    "gnode_l1_loss_f32": (_int, _L1 + [_vp, _sz, _vp]),
    "gnode_l1_loss_scaled_f32": (_int, _L1 + [C.c_float, _vp, _sz, _vp]),
    "gnode_profile_enable": (_int, [_int]),
    "gnode_profile_read": (_int, [_pf64, _pi64, _pf64, _pi64]),
    "gnode_profile_read_kind": (_int, [_i32, _pf64, _pi64]),
}
EXPORTS = list(ABI)

_lib = None


def load():
    """Load the shared library (building nothing: see gnode.build.build_lib)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GnodeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the GN-ODE path.")
    import torch  # noqa: F401  -- first, so that one HIP runtime (torch's libamdhip64.so.7) serves both
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in ABI.items():
        fn = getattr(lib, name, None)
        if fn is None:                     # an entry added without a version step: the missing symbol is the sign
            raise GnodeError(f"{LIB_PATH} is stale (no {name}): rebuild it (gnode.build.build_lib)")
        fn.restype, fn.argtypes = restype, argtypes
    if lib.gnode_version() < 226:
        raise GnodeError(f"{LIB_PATH} is stale (ABI {lib.gnode_version()} < 226): rebuild it (gnode.build.build_lib)")
    _lib = lib
    return lib


def check(status: int):
    if status != 0:
        raise GnodeError(f"libgnode_hip status {status}: {load().gnode_last_error().decode()}")


def ptr(t):
    """Device pointer of a torch tensor that must already live on the GPU, contiguous."""
    if t is None:
        return None
    if not t.is_cuda:
        raise GnodeError("GN-ODE path: tensor is not on a GPU (no CPU fallback exists)")
    if not t.is_contiguous():
        raise GnodeError("GN-ODE path: tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def host_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
