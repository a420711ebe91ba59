#!/usr/bin/env python3
"""Closed-loop timing of the sampling planner's park hint (mjpcx_set_park_hint) on the GPU: what a MOVING robot gets, as opposed to bench.py,
which plans again and again from one state (there the nominal's return equals the previous best exactly and the hint is always right).

    python tools/park_closed_loop.py [--candidates 16384] [--horizon 100] [--plans 40] [--kick-at 20] [--slacks off,0,0.02,0.05,0.1,0.2]

QuadrupedFlat from the home keyframe. Each plan: optimize_policy, then the state moves to the second state of the plan's best trajectory
(the first action applied for one planning step, by the device's own physics) and the task's transition runs at the new time. With
--kick-at K (>= 0) plan K starts from a disturbed state: 1 m/s sideways and 2 rad/s of roll added to the trunk's velocity. The loop is run
once per slack, first with `off`: MJPCX_PARK=0 in the environment while the planner's context is created and the planner's default slack,
so the library ignores the hint (the pruned launch as it was) -- the closed-loop trajectory is the same for every slack because the hint
changes no result, which the tool checks (the plans' best returns must be equal across the slacks).

Per slack one line: the mean and median wall time of optimize_policy over the plans after the first two, the event time of the rollouts
(mjpcx_timing_read), plans that needed a resume launch, candidates parked / retired by the settling pass / resumed, as shares of the batch,
and the plans for which the planner had no hint to pass (the first, and the plan after one whose resume launch held more than a quarter of
the batch)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=16384)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--plans", type=int, default=40)
    ap.add_argument("--kick-at", type=int, default=-1)
    ap.add_argument("--slacks", default="off,0,0.02,0.05,0.1,0.2")
    args = ap.parse_args()
    from bench import initial_condition
    from mujoco_mpc_amd.hostplanner import HostPlanner
    from mujoco_mpc_amd.task import load_task

    task = load_task("QuadrupedFlat")
    nq, nv = task.model.nq, task.model.nv
    H, N = args.horizon, args.candidates
    reference = None
    for slack in [s if s == "off" else float(s) for s in args.slacks.split(",")]:
        # (a planner per slack: the noise is keyed on the planner's iteration count, which a reset keeps; MJPCX_PARK is read at creation)
        if slack == "off":
            os.environ["MJPCX_PARK"] = "0"
        try:
            pl = HostPlanner(task, device=0, precision=64, seed=0, num_trajectory=N, kind="sampling")
        finally:
            os.environ.pop("MJPCX_PARK", None)
        if slack != "off":
            pl.park_set(slack)
        qpos, qvel, mocap_pos, mocap_quat = initial_condition("QuadrupedFlat", task, pl)
        pl.reset(H)
        now = 0.0
        wall, event, parked, settled, resumed, unhinted, bests = [], [], [], [], [], 0, []
        for k in range(args.plans):
            if k == args.kick_at:
                qvel = qvel.copy()
                qvel[1] += 1.0
                qvel[3] += 2.0
            pl.task_transition(now)
            pl.set_state(qpos, qvel, now, mocap_pos=mocap_pos, mocap_quat=mocap_quat)
            pl.sync()
            pl.timing_reset()
            t0 = time.perf_counter()
            pl.optimize_policy(H)
            pl.sync()
            wall.append((time.perf_counter() - t0) * 1e3)
            event.append(pl.timing_read()[0])
            info = pl.park_info()
            parked.append(info["parked"]); settled.append(info["settled_retired"]); resumed.append(info["resumed"])
            unhinted += not np.isfinite(info["hint"])
            best = pl.best_trajectory(cap=512)
            bests.append(float(best["total_return"]))
            s = np.asarray(best["states"])[1]
            qpos, qvel, now = s[:nq].copy(), s[nq:nq + nv].copy(), float(np.asarray(best["times"])[1])
        if reference is None:
            reference = bests
        assert bests == reference, "the hint changed a plan's best return"
        w, e = np.array(wall[2:]), np.array(event[2:])
        print(json.dumps({"slack": "MJPCX_PARK=0" if slack == "off" else slack, "plans": args.plans, "kick_at": args.kick_at, "candidates": N, "horizon": H,
                          "plan_ms_mean": round(float(w.mean()), 3), "plan_ms_median": round(float(np.median(w)), 3), "plan_ms_max": round(float(w.max()), 3),
                          "rollout_event_ms_mean": round(float(e.mean()), 3),
                          "plans_with_resume": int(np.count_nonzero(resumed)), "plans_without_hint": int(unhinted),
                          "parked_share": round(float(np.mean(parked)) / N, 4), "settled_retired_share": round(float(np.mean(settled)) / N, 4),
                          "resumed_share": round(float(np.mean(resumed)) / N, 4), "resumed_max": int(max(resumed)),
                          "best_return_first_last": [round(bests[0], 5), round(bests[-1], 5)]}), flush=True)
        pl.close()


if __name__ == "__main__":
    main()
