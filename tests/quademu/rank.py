"""ctypes binding of the emulator's launch in rank mode (tests/quademu/quademu_rank.cc) -- TEST INFRASTRUCTURE ONLY."""
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
        so = os.path.join(_DIR, "libquademu_rank.so")
        csrc = os.path.join(_DIR, "..", "..", "mujoco_mpc_amd", "csrc")
        srcs = [os.path.join(_DIR, "quademu_rank.cc"), os.path.join(_DIR, "quademu.cc")] + [os.path.join(csrc, f) for f in (
            "quad_step.h", "quad_model.h", "quad_abi.h", "solid_pairs.h", "pair_cull.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-o", so, srcs[0]])
        L = C.CDLL(so)
        L.quademu_rollout_ranked.argtypes = [C.POINTER(MjpcxModel), C.POINTER(MjpcxTask), c_f64p, C.c_double, c_f64p, C.c_int, C.c_int, C.c_int, C.c_int,
                                             c_f64p, c_f64p, C.c_int, C.c_int, c_f64p, C.c_int, c_i32p, c_i32p, c_i32p, c_i32p, c_f64p] + [c_f64p] * 7 + [c_i32p]
        _LIB = L
    return _LIB


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def rollout(pm, pt, state, time, mocap, N, H, P, interp, node_times, node_values, rank, nominal_candidate=0, hint=np.inf, con_cap=0):
    """N given candidates through main pass, rank bound, settling rule and resume pass. hint: one value, or one per candidate. Outputs
    start as zeros. Returns the buffers plus bound_main (the word after the main pass), bound_settle (T, what the settling rule read),
    bound (the word after the resume pass), prune_stats[4], park_step[N] (-1: never parked), resumed[N] (bool), parked / settled_retired /
    resumed_count and completed (the candidates the rank bound counted)"""
    m = pm.struct
    ds, nu, nr, ntr = m.nq + m.nv, m.nu, pt.struct.num_residual, pt.struct.num_trace
    out = dict(states=np.zeros((N, H, ds)), actions=np.zeros((N, H, nu)), times=np.zeros((N, H)), residual=np.zeros((N, H, nr)),
               costs=np.zeros((N, H)), trace=np.zeros((N, H, 3 * ntr)), total_return=np.zeros(N), failure=np.zeros(N, np.int32))
    stats, step, resumed, counts = np.zeros(4, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(4, np.int32)
    hints = _f(np.broadcast_to(np.asarray(hint, dtype=np.float64), (N,)))
    bounds = np.zeros(3)
    rc = lib().quademu_rollout_ranked(pm.ptr, pt.ptr, as_f64p(_f(state)), float(time), as_f64p(_f(mocap)), N, H, P, interp, as_f64p(_f(node_times)),
                                      as_f64p(_f(node_values)), int(nominal_candidate), int(rank), as_f64p(hints), int(con_cap), as_i32p(stats),
                                      as_i32p(step), as_i32p(resumed), as_i32p(counts), as_f64p(bounds),
                                      as_f64p(out["states"]), as_f64p(out["actions"]), as_f64p(out["times"]), as_f64p(out["residual"]),
                                      as_f64p(out["costs"]), as_f64p(out["trace"]), as_f64p(out["total_return"]), as_i32p(out["failure"]))
    if rc != 0:
        raise RuntimeError("quad kernel does not cover this model / task")
    out.update(prune_stats=stats, park_step=step, resumed=resumed.astype(bool), parked=int(counts[0]), settled_retired=int(counts[1]),
               resumed_count=int(counts[2]), completed=int(counts[3]), bound_main=float(bounds[0]), bound_settle=float(bounds[1]), bound=float(bounds[2]))
    return out


def expected(costs, H, rank, hint, nominal=0):
    """What a launch in rank mode does, as a function of the plain launch's costs (no hand-ons): per candidate the park step (-1: never;
    the first step < H - 1 whose partial return strictly exceeds the hint, never the nominal), T = the rank-th smallest return of the
    candidates that were not parked (+inf: fewer than rank), which parked candidates the settling rule retires, and per resumed candidate
    the step the resume pass retires it at against T (-1: it completes). hint: one value or one per candidate"""
    n = len(costs)
    partial = np.cumsum(costs, axis=1) / float(H)
    hints = np.broadcast_to(np.asarray(hint, dtype=np.float64), (n,))
    park = np.full(n, -1)
    for c in range(n):
        if c == nominal:
            continue
        over = np.nonzero(partial[c, :H - 1] > hints[c])[0]
        if len(over):
            park[c] = over[0]
    done = np.sort(partial[park < 0, -1])
    T = done[rank - 1] if len(done) >= rank else np.inf
    at_park = np.where(park >= 0, partial[np.arange(n), np.maximum(park, 0)], 0.0)
    retired = (park >= 0) & (at_park > T)
    resumed = (park >= 0) & ~retired
    late = np.full(n, -1)
    for c in np.nonzero(resumed)[0]:
        over = np.nonzero(partial[c, park[c]:H - 1] > T)[0]
        if len(over):
            late[c] = park[c] + over[0]
    return dict(park=park, T=float(T), retired=retired, resumed=resumed, late=late, partial=partial, completed=int((park < 0).sum()))
