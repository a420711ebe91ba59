#!/usr/bin/env python3
"""What the sampling planner's park hint (mjpcx_set_park_hint: the previous plan's best return x (1 + slack)) would park, retire and resume
in CLOSED LOOP, from the CPU oracle alone (no GPU): QuadrupedFlat from the home keyframe, sigma 0.04, 3 zero-order-hold nodes, H = 100; each
plan rolls N candidates out around the previous winner, the state then moves to the winner's second state (its first action applied for one
planning step) and the winner, resampled at the new time, is the next nominal (tools/prune_probe.py plans again and again from one state).
    python tools/park_probe.py [N = 1024] [plans = 50] [kick at plan, -1 = none] [threads = 16]
With a kick, that plan starts from a disturbed state: 1 m/s sideways and 2 rad/s of roll added to the trunk's velocity.

Per slack in {0, 0.02, 0.05, 0.1, 0.2}, over the plans after the first (which has no previous best): the share of plans that need a resume
launch, the share of candidates resumed, the mean step at which a candidate leaves its wavefront because its partial return passes the hint
(the proven bound is left out: on the device it exists only once the first wavefronts have finished; the nominal never leaves), and the mean
exit step of a wavefront of 16 consecutive candidates. A parked candidate is resumed if its partial return at the park step is not strictly
above the launch's best. The row "limit" is the launch's own FINAL best used from step 0, as prune_probe.py does: what no hint can beat."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mujoco_mpc_amd import capi  # noqa: E402
from mujoco_mpc_amd.task import load_task  # noqa: E402
from oracle import pyoracle  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
PLANS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
KICK = int(sys.argv[3]) if len(sys.argv) > 3 else -1
THREADS = int(sys.argv[4]) if len(sys.argv) > 4 else 16
H, P, SIGMA, DT = 100, 3, 0.04, 0.01
SLACKS = (None, 0.0, 0.02, 0.05, 0.1, 0.2)
MOCAP = np.array([0.3, 0, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])

task = load_task("QuadrupedFlat")
task.transition(0.0)
pm, pt = task.packed_model(), task.packed()
state = np.concatenate([task.model.keyframes["home"]["qpos"], np.zeros(18)])
shift = (H - 1) * DT / P
now, node_times, nominal = 0.0, np.arange(P) * shift, np.zeros((P, 12))
previous_best = None
rows = {s: [] for s in SLACKS}
for plan in range(PLANS):
    if plan == KICK:
        state = state.copy()
        state[19 + 1] += 1.0
        state[19 + 3] += 2.0
    ns = capi.make_noise_spec(seed=0, iteration=plan, mode=capi.NOISE_SAMPLING, std0=SIGMA)
    nodes = pyoracle.noise_candidates(pm, ns, P, nominal, np.arange(N))
    out = pyoracle.rollout_batch(pm, pt, state, now, MOCAP, N, H, P, capi.SPLINE_ZERO, node_times, nodes, num_threads=THREADS)
    ret, costs = out["total_return"], out["costs"]
    assert costs.min() >= 0
    w, best = int(ret.argmin()), float(ret.min())
    partial = np.cumsum(costs, axis=1) / H
    over = partial[:, :H - 1] > best
    over[0] = False  # the nominal is never retired or parked
    retire = np.where(over.any(axis=1), over.argmax(axis=1), H - 1)
    line = f"plan {plan:2d}: nominal {ret[0]:.4f} best {best:.4f}" + (f" previous best {previous_best:.4f} ({100 * (best / previous_best - 1):+.1f} %)" if previous_best else "")
    for s in SLACKS:
        if previous_best is None:
            continue
        if s is None:
            leave, resumed = retire, np.zeros(N, bool)
        else:
            above = partial[:, :H - 1] > previous_best * (1 + s)
            above[0] = False
            leave = np.where(above.any(axis=1), above.argmax(axis=1), H - 1)
            resumed = (leave < H - 1) & ~(partial[np.arange(N), leave] > best)
        waves = leave[:N - N % 16].reshape(-1, 16).max(axis=1)
        rows[s].append((resumed.any(), resumed.mean(), leave[1:].mean(), waves.mean()))
        if s is not None:
            line += f" | {s}: resumed {resumed.sum()}"
    print(line, flush=True)
    previous_best = best
    # closed loop: the winner's first action for one step; the winner resampled at the new time is the next nominal (zero-order hold)
    state = out["states"][w, 1].copy()
    now = float(out["times"][w, 1])
    new_times = now + np.arange(P) * shift
    index = np.clip(np.searchsorted(node_times, new_times, side="right") - 1, 0, P - 1)
    nominal, node_times = nodes[w][index].copy(), new_times
print(f"N {N}, {PLANS} plans, kick at {KICK}: slack | plans with a resume launch | candidates resumed | mean leave step | mean wavefront exit step")
for s in SLACKS:
    r = np.array(rows[s], float)
    print(f"  {'limit' if s is None else s:>7} | {100 * r[:, 0].mean():5.1f} % | {100 * r[:, 1].mean():6.2f} % | {r[:, 2].mean():5.1f} | {r[:, 3].mean():5.1f}")
