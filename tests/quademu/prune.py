"""ctypes binding of the emulator's pruned launch (tests/quademu/quademu_prune.cc) -- TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from mujoco_mpc_amd.cstructs import MjpcxModel, MjpcxTask, as_f64p, as_i32p, c_f64p, c_i32p

_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB = None
PRUNED = 0x20000000  # kQPruned (quad_abi.h) = MJPCX_FAILURE_PRUNED (mjpcx.h)


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_DIR, "libquademu_prune.so")
        csrc = os.path.join(_DIR, "..", "..", "mujoco_mpc_amd", "csrc")
        srcs = [os.path.join(_DIR, "quademu_prune.cc"), os.path.join(_DIR, "quademu.cc")] + [os.path.join(csrc, f) for f in (
            "quad_step.h", "quad_model.h", "quad_abi.h", "solid_pairs.h", "pair_cull.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-o", so, srcs[0]])
        L = C.CDLL(so)
        L.quademu_rollout_pruned.argtypes = [C.POINTER(MjpcxModel), C.POINTER(MjpcxTask), c_f64p, C.c_double, c_f64p, C.c_int, C.c_int, C.c_int, C.c_int,
                                             c_f64p, c_f64p, C.c_int, C.POINTER(C.c_uint64), c_i32p] + [c_f64p] * 7 + [c_i32p]
        _LIB = L
    return _LIB


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def rollout(pm, pt, state, time, mocap, N, H, P, interp, node_times, node_values, nominal_candidate=0, initial_bound=None):
    """N given candidates; initial_bound None: both pruning pointers null. Outputs start as zeros, so rows never written stay zero.
    Returns the buffers plus bound (the final bound) and prune_stats[4]"""
    m = pm.struct
    ds, nu, nr, ntr = m.nq + m.nv, m.nu, pt.struct.num_residual, pt.struct.num_trace
    out = dict(states=np.zeros((N, H, ds)), actions=np.zeros((N, H, nu)), times=np.zeros((N, H)), residual=np.zeros((N, H, nr)),
               costs=np.zeros((N, H)), trace=np.zeros((N, H, 3 * ntr)), total_return=np.zeros(N), failure=np.zeros(N, np.int32))
    stats = np.zeros(4, np.int32)
    bound = None if initial_bound is None else C.c_uint64(int(np.float64(initial_bound).view(np.uint64)))
    rc = lib().quademu_rollout_pruned(pm.ptr, pt.ptr, as_f64p(_f(state)), float(time), as_f64p(_f(mocap)), N, H, P, interp, as_f64p(_f(node_times)),
                                      as_f64p(_f(node_values)), int(nominal_candidate), None if bound is None else C.byref(bound), as_i32p(stats),
                                      as_f64p(out["states"]), as_f64p(out["actions"]), as_f64p(out["times"]), as_f64p(out["residual"]),
                                      as_f64p(out["costs"]), as_f64p(out["trace"]), as_f64p(out["total_return"]), as_i32p(out["failure"]))
    if rc != 0:
        raise RuntimeError("quad kernel does not cover this model / task")
    out["prune_stats"] = stats
    out["bound"] = None if bound is None else float(np.uint64(bound.value).view(np.float64))
    return out
