"""ctypes binding of the emulator's launch with a park hint (tests/quademu/quademu_park.cc) -- TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from mujoco_mpc_amd.cstructs import MjpcxModel, MjpcxTask, as_f64p, as_i32p, c_f64p, c_i32p

_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB = None
FALLBACK = 0x40000000  # kQFallback (quad_abi.h)
PRUNED = 0x20000000    # kQPruned
PARKED = 0x10000000    # kQParked: never left in failure[] once the settling rule has run


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_DIR, "libquademu_park.so")
        csrc = os.path.join(_DIR, "..", "..", "mujoco_mpc_amd", "csrc")
        srcs = [os.path.join(_DIR, "quademu_park.cc"), os.path.join(_DIR, "quademu.cc")] + [os.path.join(csrc, f) for f in (
            "quad_step.h", "quad_model.h", "quad_abi.h", "solid_pairs.h", "pair_cull.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-o", so, srcs[0]])
        L = C.CDLL(so)
        L.quademu_rollout_parked.argtypes = [C.POINTER(MjpcxModel), C.POINTER(MjpcxTask), c_f64p, C.c_double, c_f64p, C.c_int, C.c_int, C.c_int, C.c_int,
                                             c_f64p, c_f64p, C.c_int, C.POINTER(C.c_uint64), c_f64p, C.c_int, C.c_int, c_i32p, c_i32p, c_i32p, c_i32p,
                                             c_f64p] + [c_f64p] * 7 + [c_i32p]
        _LIB = L
    return _LIB


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def rollout(pm, pt, state, time, mocap, N, H, P, interp, node_times, node_values, nominal_candidate=0, initial_bound=np.inf, hint=np.inf,
            resume_unpruned=False, con_cap=0):
    """N given candidates through main pass, settling rule and resume pass. hint: one value, or one per candidate. initial_bound None: a plain launch (no bound word: nothing retired or parked). Outputs start as zeros.
    Returns the buffers plus bound (final), bound_settle (what the settling rule read), prune_stats[4], park_step[N] (-1: never parked),
    resumed[N] (bool) and parked / settled_retired / resumed_count"""
    m = pm.struct
    ds, nu, nr, ntr = m.nq + m.nv, m.nu, pt.struct.num_residual, pt.struct.num_trace
    out = dict(states=np.zeros((N, H, ds)), actions=np.zeros((N, H, nu)), times=np.zeros((N, H)), residual=np.zeros((N, H, nr)),
               costs=np.zeros((N, H)), trace=np.zeros((N, H, 3 * ntr)), total_return=np.zeros(N), failure=np.zeros(N, np.int32))
    stats, step, resumed, counts = np.zeros(4, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(3, np.int32)
    hints = _f(np.broadcast_to(np.asarray(hint, dtype=np.float64), (N,)))
    bound = None if initial_bound is None else C.c_uint64(int(np.float64(initial_bound).view(np.uint64)))
    settle = np.zeros(1)
    rc = lib().quademu_rollout_parked(pm.ptr, pt.ptr, as_f64p(_f(state)), float(time), as_f64p(_f(mocap)), N, H, P, interp, as_f64p(_f(node_times)),
                                      as_f64p(_f(node_values)), int(nominal_candidate), None if bound is None else C.byref(bound), as_f64p(hints), int(bool(resume_unpruned)),
                                      int(con_cap), as_i32p(stats), as_i32p(step), as_i32p(resumed), as_i32p(counts), as_f64p(settle),
                                      as_f64p(out["states"]), as_f64p(out["actions"]), as_f64p(out["times"]), as_f64p(out["residual"]),
                                      as_f64p(out["costs"]), as_f64p(out["trace"]), as_f64p(out["total_return"]), as_i32p(out["failure"]))
    if rc != 0:
        raise RuntimeError("quad kernel does not cover this model / task")
    out.update(prune_stats=stats, park_step=step, resumed=resumed.astype(bool), parked=int(counts[0]), settled_retired=int(counts[1]),
               resumed_count=int(counts[2]), bound=None if bound is None else float(np.uint64(bound.value).view(np.float64)), bound_settle=float(settle[0]))
    return out
