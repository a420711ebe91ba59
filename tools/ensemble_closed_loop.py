#!/usr/bin/env python3
"""Closed loop on a robot whose model the planner is NOT told: does planning over an ensemble of model hypotheses drive it better than
planning on the nominal model with the same number of rollouts?

    python tools/ensemble_closed_loop.py [--steps 60] [--horizon 100] [--true-payload 0.45] [--payloads 0,0.1,0.2,0.3,0.4,0.5,0.6,0.7]
                                         [--tail 8] [--seed 0] [--out profiles/ensemble_closed_loop.jsonl]

The plant is an A1 (QuadrupedFlat, from the home keyframe) on a context created on the TRUE model: the task's model with a payload --
the trunk's mass and inertia x (1 + true-payload) -- which no planner sees. It is stepped as the reference's testspeed steps its
simulation: one candidate, two steps (mjpcx_rollout_splines with the action held), the second state is the robot's next state and the
first step's cost is what the robot paid. Two controllers drive it, each from the same start, replanning before every step:

    sampling   GpuSamplingPlanner on the BASE model, 16384 candidates
    ensemble   GpuEnsembleSamplingPlanner over the payload hypotheses (--payloads: trunk x (1 + p) each; the true one is not among them),
               16384 / M candidates each (8 x 2048), score = the mean of the --tail largest returns (M: the mean; 1: the worst case)

Per controller one JSON line: the closed-loop cost summed along the run (and its mean per step), the ms per plan (median, min, max over the
plans after the first two) and whether the robot fell (trunk height below 0.15 m at any step). The tool reports; it asserts nothing
about which controller wins."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def payload(mjcf, m, p):
    trunk = int(np.flatnonzero(np.asarray(m.arrays["body_dofnum"]) > 0)[0])
    mass, inertia = np.array(m.arrays["body_mass"], float), np.array(m.arrays["body_inertia"], float)
    mass[trunk] *= 1.0 + p
    inertia[trunk] *= 1.0 + p
    return mjcf.variant(m, body_mass=mass, body_inertia=inertia)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--candidates", type=int, default=16384, help="rollouts per plan, for both controllers")
    ap.add_argument("--true-payload", type=float, default=0.45)
    ap.add_argument("--payloads", default="0,0.1,0.2,0.3,0.4,0.5,0.6,0.7")
    ap.add_argument("--tail", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--controllers", default="sampling,ensemble")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mujoco_mpc_amd import capi, mjcf
    from mujoco_mpc_amd.cstructs import PackedModel
    from mujoco_mpc_amd.planners import GpuEnsembleSamplingPlanner, GpuSamplingPlanner, State, sync_task
    from mujoco_mpc_amd.task import load_task

    task = load_task("QuadrupedFlat")
    task.transition(0.0)
    m = task.model
    H, nq = args.horizon, m.nq
    hyp = [float(x) for x in args.payloads.split(",")]
    M = len(hyp)
    if args.true_payload in hyp:
        raise SystemExit("ensemble_closed_loop.py: the true payload is one of the hypotheses; the planner must not be told the true model")
    if args.candidates % (64 * M):
        raise SystemExit(f"ensemble_closed_loop.py: --candidates must be a multiple of 64 x {M} hypotheses")
    ts, integ = m.get_number("agent_timestep", m.timestep), int(m.get_number("agent_integrator", m.integrator))
    plant = capi.Context(PackedModel(payload(mjcf, m, args.true_payload), timestep=ts, integrator=integ), task.packed(), 0, 64)
    home = np.asarray(m.keyframes["home"]["qpos"], float)
    goal, quat = np.array([[0.3, 0, 0.26], [-2.5, 0, 0]]), np.array([[1.0, 0, 0, 0]] * 2)
    lines = []
    for kind in args.controllers.split(","):
        if kind == "sampling":
            pl = GpuSamplingPlanner(seed=args.seed)
            pl.initialize(m, task)
            pl.num_trajectory_ = args.candidates
            pl.allocate()
        else:
            pl = GpuEnsembleSamplingPlanner(M, seed=args.seed, tail=args.tail)
            pl.initialize(m, task)
            pl.num_trajectory_ = args.candidates // M
            pl.allocate()
            pl.set_models([payload(mjcf, m, p) for p in hyp])
        pl.reset(H)
        st = State(m)
        st.set(home, np.zeros(m.nv), mocap_pos=goal, mocap_quat=quat, time=0.0)
        wall, costs, fell = [], [], False
        for k in range(args.steps):
            pl.set_state(st)
            t0 = time.perf_counter()
            pl.optimize_policy(H)
            wall.append((time.perf_counter() - t0) * 1e3)
            action = pl.action_from_policy(np.zeros(m.nu), None, st.time)
            sync_task(plant, task)
            plant.set_state(st.state, st.time, st.mocap, st.userdata)
            plant.rollout_splines(2, capi.SPLINE_ZERO, np.array([st.time]), np.asarray(action, float).reshape(1, 1, m.nu))
            tr = plant.fetch_trajectory(0)
            costs.append(float(tr.costs[0]))
            fell = fell or bool(tr.failure) or float(tr.states[1, 2]) < 0.15
            st.set(tr.states[1, :nq], tr.states[1, nq:], mocap_pos=goal, mocap_quat=quat, time=float(tr.times[1]))
        pl.ctx.close()
        w = np.array(wall[2:] if len(wall) > 2 else wall)
        rec = {"tool": "ensemble_closed_loop", "controller": kind, "true_payload": args.true_payload, "steps": args.steps, "horizon": H,
               "rollouts_per_plan": args.candidates, "seed": args.seed, "closed_loop_cost": float(np.sum(costs)), "cost_per_step": float(np.mean(costs)),
               "cost_last_quarter_per_step": float(np.mean(costs[-max(args.steps // 4, 1):])), "fell": fell,
               "plan_ms": {"median": float(np.median(w)), "min": float(w.min()), "max": float(w.max())}}
        if kind != "sampling":
            rec.update(hypotheses=hyp, tail=pl.tail)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    plant.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
