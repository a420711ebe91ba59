#!/usr/bin/env python3
"""Closed-loop timing of a fleet's pruned plan step (GpuBatchSamplingPlanner.pruning, mjpcx_set_pruning_batched) on the GPU: E MOVING
robots, as tools/park_closed_loop.py does for one. tools/batch_sweep.py --prune plans again and again from the same states, where every
robot's nominal return equals its previous best and the hint is always right; a hint only earns its keep on robots that move.

    python tools/fleet_closed_loop.py [--envs 8] [--candidates 2048] [--horizon 100] [--plans 24] [--modes off,prune,hints]
                                      [--planner cross_entropy] [--slack 0.05]

QuadrupedFlat, every robot from the home keyframe with a heading goal of its own and noise stream seed + e. Each plan: optimize_policy, then
every robot moves to the second state of its plan's best trajectory. The loop runs once per mode on a fresh planner: `off` (pruning False),
`prune` (bounds only: park_slack = -1), `hints` (the planner's default slack). The closed-loop trajectories are the same in every mode
because neither bounds nor hints change a result, which the tool checks (every plan's best returns must be equal across the modes).

Per mode one JSON line: median (min, max) wall ms of optimize_policy over the plans after the first two, and per robot the shares of its
candidates retired, parked and resumed and the number of plans it had no hint for."""
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
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--candidates", type=int, default=2048)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--plans", type=int, default=24)
    ap.add_argument("--modes", default="off,prune,hints")
    ap.add_argument("--planner", choices=["sampling", "cross_entropy"], default="sampling",
                    help="cross_entropy: GpuBatchCrossEntropyPlanner (rank mode: the launch settles on the (n_elite + 1)-th return); --candidates then counts the nominal rollout")
    ap.add_argument("--slack", type=float, default=None, help="mode hints: the park slack (default: the planner's own)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mujoco_mpc_amd.planners import GpuBatchCrossEntropyPlanner, GpuBatchSamplingPlanner, State
    from mujoco_mpc_amd.task import load_task

    task = load_task("QuadrupedFlat")
    task.transition(0.0)
    m = task.model
    E, n, H = args.envs, args.candidates, args.horizon
    home = np.asarray(m.keyframes["home"]["qpos"], float)
    reference, lines = None, []
    for mode in args.modes.split(","):
        ce = args.planner == "cross_entropy"
        pl = (GpuBatchCrossEntropyPlanner if ce else GpuBatchSamplingPlanner)(E, seed=0)
        pl.initialize(m, task)
        pl.num_trajectory_ = n - 1 if ce else n   # (the Cross-Entropy fleet's nominal rollout rides along as each robot's last candidate)
        if ce:
            pl.n_elite_ = max((n - 1) // 10, 2)
        pl.allocate()
        pl.pruning = mode != "off"
        if mode == "prune":
            pl.park_slack = -1.0
        elif args.slack is not None:
            pl.park_slack = args.slack
        pl.reset(H)
        goals = [np.array([[0.3 * np.cos(0.7 * e), 0.3 * np.sin(0.7 * e), 0.26], [-2.5, 0, 0]]) for e in range(E)]
        quat = np.array([[1.0, 0, 0, 0]] * 2)
        states = []
        for e in range(E):
            st = State(m)
            st.set(home, np.zeros(m.nv), mocap_pos=goals[e], mocap_quat=quat, time=0.0)
            states.append(st)
        wall, bests = [], []
        sums = {k: np.zeros(E) for k in ("retired", "parked", "resumed")}
        unhinted = np.zeros(E, int)
        for k in range(args.plans):
            pl.set_states(states)
            t0 = time.perf_counter()
            pl.optimize_policy(H)
            wall.append((time.perf_counter() - t0) * 1e3)
            bests.append([(p.improvement, tuple(p.trajectory_order)) if ce else p.best_return for p in pl.envs])
            if pl.prune_stats is not None and k >= 2:
                sums["retired"] += pl.prune_stats["retired"]
                sums["parked"] += pl.park_stats["parked"]
                sums["resumed"] += pl.park_stats["resumed"]
                unhinted += np.isinf(pl.park_hints_used)
            for e in range(E):
                tr = pl.best_trajectory(e)
                states[e].set(tr.states[1, :m.nq], tr.states[1, m.nq:], mocap_pos=goals[e], mocap_quat=quat, time=float(tr.times[1]))
        pl.ctx.close()
        if reference is None:
            reference = bests
        elif bests != reference:
            raise SystemExit(f"fleet_closed_loop.py: mode {mode} planned differently from mode {args.modes.split(',')[0]}: pruning changed a result")
        w = np.array(wall[2:])
        share = lambda x: [round(float(v) / (n * max(args.plans - 2, 1)), 4) for v in x]
        rec = {"tool": "fleet_closed_loop", "planner": args.planner, "park_slack": pl.park_slack, "mode": mode, "num_envs": E, "n_per_env": n, "horizon": H, "plans": args.plans,
               "plan_ms": {"median": float(np.median(w)), "min": float(w.min()), "max": float(w.max())},
               "retired_share": share(sums["retired"]), "parked_share": share(sums["parked"]), "resumed_share": share(sums["resumed"]),
               "plans_without_hint": [int(v) for v in unhinted]}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
