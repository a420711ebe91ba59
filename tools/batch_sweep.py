#!/usr/bin/env python3
"""What many environments per launch buy: for each shape E x n, the time of (a) E sequential plan steps (set_state, rollout_noise, best:
each ends in its own sync) and (b) one batched plan step (set_states, rollout_noise_batched, best_batched: one sync) on the same context,
alternating in one process. Host clock around work that ends in a sync; warm-up for every shape; median and spread over the timed steps.

  python tools/batch_sweep.py [--steps 12] [--warmup 2] [--out profiles/batch_sweep.jsonl] [--only QuadrupedFlat] [--shapes 8x2048,1x16384]

--planner cross_entropy: the Cross-Entropy plan step instead. (a) per environment set_state, rollout_noise (CE), topk, elite_moments twice
-- four round trips, three of them syncs -- against (b) set_states, rollout_noise_batched_ce with a variance row per environment and
ce_update_batched: one sync. n counts the nominal rollout (the last candidate of every environment), n_elite = n / 10. The record also
splits the batched step, in a loop of its own: the rollout up to its sync, and the update call alone (launch + sync) after it. Default
output profiles/batch_sweep_ce.jsonl.

--planner gradient: the Gradient planner's plan step. (a) E GpuGradientPlanner plan steps on one context, one after the other (nominal
rollout, transition_fd, cost_derivatives, gradient_pass, line-search rollout: six round trips per robot) against (b) one
GpuBatchGradientPlanner plan step (rollout_splines_batched, gradient_step_batched, rollout_splines_batched, returns: two syncs for the
fleet), host logic included on both sides, 64 line-search candidates per environment. The record carries the batched planner's stage
timers (medians). Default output profiles/batch_sweep_gradient.jsonl.

--planner ilqg: the iLQG plan step on the A1 (T = 36, 10 rollouts). (a) E GpuILQGPlanner plan steps on one context, one after the other,
against (b) one GpuBatchILQGPlanner plan step: the nominal and the line-search rollouts of the fleet in one rollout_feedback_batched
launch each, the derivative chain and the Riccati pass with its retries in one ilqg_step_batched between them (--no-device-chain: per
environment on the plain calls, the planner's device_chain = False; `device_chain` in the record says which ran). Host logic included on
both sides. The record carries the batched planner's stage timers (medians; median / min / max under batched_stage_spread_ms) and one
environment's sequential ones. Default output profiles/batch_sweep_ilqg.jsonl.

--planner robust: the Robust planner's plan step, k = 16 candidates x R = 4 repetitions (--robust 16x4). (a) E GpuRobustPlanner plan steps,
one after the other, on two contexts (the delegate's rollout, topk, k spline fetches, the noisy rollout of k x R replicated splines,
returns, the host loop: per robot) against (b) one GpuBatchRobustPlanner plan step on the same two contexts (rollout_noise_batched and
robust_step_batched: two launch sequences, one sync). Host logic included on both sides. Default output profiles/batch_sweep_robust.jsonl.

--planner sample_gradient: the Sample-Gradient planner's plan step, G = 32 gradient candidates (--gradient-candidates 32). (a) E
GpuSampleGradientPlanner plan steps, one after the other, each on a context of its own (the gradient candidates and the shaping weights
live in the context: one per robot) against (b) one GpuBatchSampleGradientPlanner plan step on one context
(rollout_sample_gradient_batched and sample_gradient_update_batched: one sync for the fleet). Host logic included on both sides. The
record also splits the batched step, in a loop of its own: the rollout call up to its sync (candidate kernel + rollout), and the update
call alone (launch + sync) after it. Default output profiles/batch_sweep_sample_gradient.jsonl.

--planner ilqs: the iLQS plan step on the A1 (T = 36, 64 sampling candidates, 10 iLQG rollouts), three variants alternating in one
process on the same two contexts (sampling, iLQG): (a) E GpuILQSPlanner plan steps, one after the other; (b) one GpuBatchILQSPlanner plan
step -- nominal rollouts, sampling, one ilqg_step_batched_from that gathers every member's nominal from the context that holds it, the
line search; (c) the same fleet with device_chain = False (the members' sequential chains through host memory). --no-device-chain: (b)
runs without the chain too and (c) is left out. Host logic included on every side. The record carries each fleet's stage timers
(nominal, fit, sampling, handoff, derivatives_backward, rollouts: medians and spread) and, per timed step, how many members were in the
nominal phase, went on to iLQG and were gathered from the sampling context, with that step's time and its derivatives_backward (the
fleet's composition moves while robots migrate to iLQG: --warmup 16 times a settled fleet). Default output profiles/batch_sweep_ilqs.jsonl.

--planner ensemble: the ensemble plan step -- ONE robot, E hypotheses about its model (--mixed-models; without it E copies of one model), n
shared candidates. Two variants alternating in one session on one context, from the same states and nominal: (a) "sampling", the fleet's plan
step as above (set_states, rollout_noise_batched, best_batched); (b) "ensemble": set_states, rollout_noise_ensemble, ensemble_best (--tail,
default E: the mean). The same launch over E x n rollouts with the noise stream shared, and ensemble_best in place of best_batched: the
expectation is equal times. Default shape 8 x 2048 on the A1, H = 100, fp64; default output profiles/batch_sweep_ensemble.jsonl.

--planner cmaes: the CMA-ES plan step (set_states, rollout_cma_batched, cma_update_batched; Hansen's defaults, sigma0 the model's
sampling_exploration, the returned mean the next nominal, the distribution moving on from step to step; once with sigma free in
[1e-6, 2] and once with sigma held at sampling_exploration) against the unpruned Predictive Sampling plan step of the same fleet,
alternating as for --planner mppi; then the candidate kernel (the first kernel of the rollout's launch) and the update alone under the
context's timer. Default shapes as for mppi; default output
profiles/batch_sweep_cmaes.jsonl.

--planner mppi: the MPPI plan step against the unpruned Predictive Sampling plan step of the same fleet. Two variants alternating in one
session on one context, from the same states and nominal, for --rounds rounds (default 2) of --steps timed steps each: (a) "sampling":
set_states, rollout_noise_batched, best_batched; (b) "mppi": set_states, rollout_noise_batched, mppi_update_batched. The launch is the same;
the update differs. Afterwards the update alone, --steps times under the context's timer: its two kernels' time (timing_read) and its first
kernel's, the weights (timing_read_main). --temperature X (default: the spread of environment 0's returns in the first warm-up launch over
10; the time does not depend on it). MPPI needs every return, so it cannot prune: the PRUNED sampling step (--planner sampling --prune) is
faster than either side here. Default shapes 8 x 2048 and 1 x 16384 on the A1, H = 100, fp64; default output profiles/batch_sweep_mppi.jsonl.

--mixed-params: every environment plans with task weights, norm parameters, residual parameters and risk of its own (sampling and
cross_entropy: set_task_params_batched after set_states, and the plain set_task_params of the same row before every sequential plan
step; gradient and ilqg: the fleet planner's set_tasks, and every sequential planner on its own task). The kernels do the same work
either way; the record carries "mixed_params". Compare with the same run without the switch.

--mixed-models (sampling and cross_entropy, the contact tasks): every environment rolls out on a model of its own -- payload, friction and
actuator-strength variations of the robot (mjcf.variant), handed to the context once per shape with set_models_batched (the record
carries that call's time, "set_models_ms": the builders run once per model on the host -- a setup call). The sequential side then plans
on E contexts, each created on its environment's model. The kernels do the same work either way; compare with the same run without
the switch.

Kernel thresholds are the library's defaults: the sequential side of 8 x 2048 runs eight launches of the kernel a 2048-candidate batch gets,
the batched side one launch of the kernel a 16384-candidate batch gets -- that is the feature."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mujoco_mpc_amd import capi  # noqa: E402
from mujoco_mpc_amd.task import load_task  # noqa: E402

# (task, precision, horizon, [(E, n), ...])
SHAPES = [("QuadrupedFlat", 64, 100, [(8, 2048), (4, 4096), (1, 16384)]),
          ("HumanoidTrack", 32, 64, [(4, 2048), (1, 8192)]),
          ("Cartpole", 64, 128, [(64, 64), (1, 4096)])]


def initial(task, name, E, rng):
    """E states (perturbed around the task's start), clocks and mocap poses"""
    m = task.model
    if name == "QuadrupedFlat":
        task.transition(0.0)
        q0, v0 = np.asarray(m.keyframes["home"]["qpos"], float), np.zeros(m.nv)
        mocap = np.array([0.3, 0, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])
    elif name == "HumanoidTrack":
        e = task.transition(0.0, mode=9)
        q0, v0 = np.asarray(e["qpos"], float), np.asarray(e["qvel"], float)
        mocap = np.concatenate([np.concatenate([p, [1, 0, 0, 0]]) for p in np.asarray(e["mocap_pos"]).reshape(-1, 3)])
    else:
        q0, v0, mocap = np.zeros(m.nq), np.zeros(m.nv), None
    states = []
    for e in range(E):
        q = q0.copy()
        if name == "Cartpole":
            q += rng.uniform(-0.5, 0.5, m.nq)
        else:
            q[7:] += rng.normal(0, 0.02, m.nq - 7)   # joints only: the base pose and its quaternion stay
        states.append(np.concatenate([q, v0]))
    return np.stack(states), np.zeros(E), None if mocap is None else np.stack([mocap] * E)


def mixed_tasks(task, E):
    """E copies of the task (sharing its model) with their own weights (x 0.5 .. 2), norm parameters (x 0.7 .. 1.5), residual parameters
    that are not selections (x 0.8 .. 1.2, + 0.01 .. 0.1) and risk (0 and 0.2 in turn)"""
    import copy
    rng = np.random.default_rng(5)
    names = [k for k in task.model.numeric if k.startswith("residual_")]
    out = []
    for e in range(E):
        t = copy.copy(task)
        t.weight = [float(w * f) for w, f in zip(task.weight, rng.uniform(0.5, 2.0, len(task.weight)))]
        t.norm_parameter = [float(p * f) for p, f in zip(task.norm_parameter, rng.uniform(0.7, 1.5, len(task.norm_parameter)))]
        t.parameters = [float(v) if k.startswith("residual_select_") else float(v * rng.uniform(0.8, 1.2) + rng.uniform(0.01, 0.1))
                        for k, v in zip(names, task.parameters)]
        t.risk = 0.2 * (e % 2)
        out.append(t)
    return out


def mixed_models(task, E):
    """E packed models of the task's robot: the model itself, then in turn a payload on the first moving body (+ 10 % .. of its mass and
    inertia per robot), a slipperier world (sliding friction x 0.9 ..) and weaker actuators (x 0.95 ..), growing with the robot's number"""
    from mujoco_mpc_amd import mjcf
    from mujoco_mpc_amd.cstructs import PackedModel
    m = task.model
    a = {k: np.asarray(m.arrays[k], float) for k in ("body_mass", "body_inertia", "geom_friction", "actuator_gear", "actuator_gainprm")}
    trunk = int(np.flatnonzero(np.asarray(m.arrays["body_dofnum"]) > 0)[0])
    gain = "actuator_gainprm" if np.any(np.asarray(m.arrays["actuator_biastype"]) == 0) and np.unique(a["actuator_gear"]).size == 1 else "actuator_gear"
    ts, integ = m.get_number("agent_timestep", m.timestep), int(m.get_number("agent_integrator", m.integrator))
    out = []
    for e in range(E):
        mass, inertia, friction, act = a["body_mass"].copy(), a["body_inertia"].copy(), a["geom_friction"].copy(), a[gain].copy()
        step = 1 + e // 4
        if e % 4 == 1:
            mass[trunk] *= 1 + 0.1 * step
            inertia[trunk] *= 1 + 0.1 * step
        elif e % 4 == 2:
            friction.reshape(-1, 3)[:, 0] *= 0.9 ** step
        elif e % 4 == 3:
            act.reshape(len(act), -1)[:, 0] *= 0.95 ** step
        fm = m if e == 0 else mjcf.variant(m, body_mass=mass, body_inertia=inertia, geom_friction=friction, **{gain: act})
        out.append(PackedModel(fm, timestep=ts, integrator=integ))
    return out


def task_rows(tasks):
    arr = lambda k: np.array([getattr(t, k) for t in tasks], float).reshape(len(tasks), -1)
    return dict(weight=arr("weight"), norm_parameter=arr("norm_parameter"), parameters=arr("parameters"), risk=np.array([float(t.risk) for t in tasks]))


ENSEMBLE_SHAPES = [("QuadrupedFlat", 64, 100, [(8, 2048)])]


def sweep_ensemble(name, precision, H, shapes, steps, warmup, out, tail=None, models=False):
    task = load_task(name)
    m = task.model
    rng = np.random.default_rng(1)
    ctx = capi.Context(task.packed_model(), task.packed(), 0, precision)
    P = int(m.get_number("sampling_spline_points", 6))
    interp = int(m.get_number("sampling_representation", capi.SPLINE_CUBIC))
    std = float(m.get_number("sampling_exploration", 0.1))
    dt = m.get_number("agent_timestep", m.timestep)
    times1 = np.arange(P) * ((H - 1) * dt / max(P - 1, 1))
    for E, n in shapes:
        raw, clocks, mocap = initial(task, name, 1, rng)
        states, clocks, mocap = np.repeat(raw, E, axis=0), np.repeat(clocks, E), None if mocap is None else np.repeat(mocap, E, axis=0)   # the one robot
        times, nominal = np.stack([times1] * E), np.zeros((E, P, m.nu))
        k = E if tail is None else int(tail)
        if models:
            ctx.set_models_batched(mixed_models(task, E))
        it = [0]

        def sampling():
            it[0] += 1
            ctx.set_states(states, clocks, mocap)
            ctx.rollout_noise_batched(n, H, interp, times, nominal, capi.make_noise_spec(seed=7, iteration=it[0], std0=std), num_envs=E)
            ctx.best_batched(E, 0)

        def ensemble():
            ctx.set_states(states, clocks, mocap)
            ctx.rollout_noise_ensemble(n, H, interp, times1, nominal[0], capi.make_noise_spec(seed=7, iteration=it[0], std0=std), num_hypotheses=E)
            ctx.ensemble_best(E, k, 0)

        for _ in range(warmup):
            sampling()
            ensemble()
        ta, tb = [], []
        for _ in range(steps):   # alternating: both sides see the same clocks and the same neighbours on the machine
            t0 = time.perf_counter(); sampling(); t1 = time.perf_counter(); ensemble(); t2 = time.perf_counter()
            ta.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
        rec = {"planner": "ensemble", "task": name, "precision": precision, "horizon": H, "num_hypotheses": E, "n": n, "tail": k, "steps": steps,
               "warmup": warmup, "mixed_models": bool(models), "kernel": ctx.kernel_name.split(" (")[0], "sampling_ms": stats(ta), "ensemble_ms": stats(tb),
               "ratio_ensemble_over_sampling": float(np.median(tb) / np.median(ta)),
               "inside_spread": bool(np.min(ta) <= np.median(tb) <= np.max(ta))}
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()
        if models:
            ctx.set_models_batched(None)
    ctx.close()


MPPI_SHAPES = [("QuadrupedFlat", 64, 100, [(8, 2048), (1, 16384)])]


def sweep_mppi(name, precision, H, shapes, steps, warmup, out, temperature=None, rounds=2):
    task = load_task(name)
    m = task.model
    rng = np.random.default_rng(1)
    ctx = capi.Context(task.packed_model(), task.packed(), 0, precision)
    P = int(m.get_number("sampling_spline_points", 6))
    interp = int(m.get_number("sampling_representation", capi.SPLINE_CUBIC))
    std = float(m.get_number("sampling_exploration", 0.1))
    dt = m.get_number("agent_timestep", m.timestep)
    times1 = np.arange(P) * ((H - 1) * dt / max(P - 1, 1))
    for E, n in shapes:
        states, clocks, mocap = initial(task, name, E, rng)
        times, nominal = np.stack([times1] * E), np.zeros((E, P, m.nu))
        it = [0]
        lam = [temperature]
        last = {}

        def launch():
            ctx.set_states(states, clocks, mocap)
            ctx.rollout_noise_batched(n, H, interp, times, nominal, capi.make_noise_spec(seed=7, iteration=it[0], std0=std), num_envs=E)

        def sampling():
            it[0] += 1
            launch()
            ctx.best_batched(E, 0)

        def mppi():
            launch()
            if lam[0] is None:
                r = ctx.returns()[0][:n]
                r = r[np.isfinite(r) & (r < 1e6)]
                lam[0] = max(float(r.max() - r.min()) / 10.0, 1e-12)
            last.update(ctx.mppi_update_batched(E, lam[0], 0))

        for _ in range(warmup):
            sampling()
            mppi()
        per_round = []
        for _ in range(rounds):
            ta, tb = [], []
            for _ in range(steps):   # alternating: both sides see the same clocks and the same neighbours on the machine
                t0 = time.perf_counter(); sampling(); t1 = time.perf_counter(); mppi(); t2 = time.perf_counter()
                ta.append((t1 - t0) * 1e3)
                tb.append((t2 - t1) * 1e3)
            per_round.append({"sampling_ms": stats(ta), "mppi_ms": stats(tb)})
        # the update alone on the last launch: wall time, and its kernels' under the context's timer
        tu = []
        ctx.timing_reset()
        for _ in range(steps):
            t0 = time.perf_counter(); ctx.mppi_update_batched(E, lam[0], 0); tu.append((time.perf_counter() - t0) * 1e3)
        first_ms, _ = ctx.timing_read_main()
        both_ms, calls = ctx.timing_read()
        med = lambda k: [r[k]["median"] for r in per_round]
        rec = {"planner": "mppi", "task": name, "precision": precision, "horizon": H, "num_envs": E, "n_per_env": n, "steps": steps, "warmup": warmup,
               "rounds": per_round, "temperature": lam[0], "kernel": ctx.kernel_name.split(" (")[0],
               "effective_samples": [float(x) for x in last["effective_samples"]],
               "ratio_mppi_over_sampling": [float(b / a) for a, b in zip(med("sampling_ms"), med("mppi_ms"))],
               "sampling_spread_between_rounds_ms": float(max(med("sampling_ms")) - min(med("sampling_ms"))),
               "update_call_ms": stats(tu), "update_kernels_ms": both_ms / max(calls, 1), "update_weights_kernel_ms": first_ms / max(calls, 1),
               "update_mean_kernel_ms": (both_ms - first_ms) / max(calls, 1)}
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()
    ctx.close()


def sweep_cmaes(name, precision, H, shapes, steps, warmup, out, rounds=2):
    """the CMA-ES plan step against the unpruned Predictive Sampling plan step of the same fleet, alternating (as sweep_mppi), in two
    variants one after the other: "adaptive" (sigma free in [1e-6, 2], as the planner's defaults) and "fixed_sigma" (sigma held at the
    model's sampling_exploration, so the candidates are as far from the mean as Predictive Sampling's: the cost of the mechanism alone).
    As in the planner the returned mean is the next step's nominal; the states stay where they are."""
    from mujoco_mpc_amd.planners import cma_parameters
    task = load_task(name)
    m = task.model
    rng = np.random.default_rng(1)
    ctx = capi.Context(task.packed_model(), task.packed(), 0, precision)
    P = int(m.get_number("sampling_spline_points", 6))
    interp = int(m.get_number("sampling_representation", capi.SPLINE_CUBIC))
    std = float(m.get_number("sampling_exploration", 0.1))
    dt = m.get_number("agent_timestep", m.timestep)
    times1 = np.arange(P) * ((H - 1) * dt / max(P - 1, 1))
    d = P * m.nu
    for E, n in shapes:
        states, clocks, mocap = initial(task, name, E, rng)
        times, zeros = np.stack([times1] * E), np.zeros((E, P, m.nu))
        defaults = cma_parameters(d, n - 1)
        rec = {"planner": "cmaes", "task": name, "precision": precision, "horizon": H, "num_envs": E, "n_per_env": n, "steps": steps, "warmup": warmup,
               "num_params": d, "mu": int(defaults["mu"]), "kernel": ctx.kernel_name.split(" (")[0], "sigma0": std}
        for variant, lo, hi in (("adaptive", 1e-6, 2.0), ("fixed_sigma", std, std)):
            prm = dict(defaults, sigma_min=lo, sigma_max=hi, pivot_floor=1e-12)
            it = [0]
            last = {}
            mean = [zeros.copy()]
            ctx.set_states(states, clocks, mocap)
            ctx.cma_set_state_batched(E, d, std)

            def sampling():
                it[0] += 1
                ctx.set_states(states, clocks, mocap)
                ctx.rollout_noise_batched(n, H, interp, times, zeros, capi.make_noise_spec(seed=7, iteration=it[0], std0=std), num_envs=E)
                ctx.best_batched(E, 0)

            def cmaes():
                ctx.set_states(states, clocks, mocap)
                ctx.rollout_cma_batched(n, H, interp, times, mean[0], seed=7, iteration=it[0], num_envs=E)
                last.update(ctx.cma_update_batched(E, prm))
                mean[0] = last["mean"].copy()

            for _ in range(warmup):
                sampling()
                cmaes()
            per_round = []
            for _ in range(rounds):
                ta, tb, sig = [], [], []
                for _ in range(steps):   # alternating: both sides see the same clocks and the same neighbours on the machine
                    t0 = time.perf_counter(); sampling(); t1 = time.perf_counter(); cmaes(); t2 = time.perf_counter()
                    ta.append((t1 - t0) * 1e3)
                    tb.append((t2 - t1) * 1e3)
                    sig.append(float(np.max(last["sigma"])))
                per_round.append({"sampling_ms": stats(ta), "cmaes_ms": stats(tb), "largest_sigma": stats(sig)})
            # the candidate kernel: the first kernel of the rollout's launch under the context's timer
            ctx.timing_reset()
            for _ in range(steps):
                ctx.set_states(states, clocks, mocap)
                ctx.rollout_cma_batched(n, H, interp, times, mean[0], seed=7, iteration=it[0], num_envs=E)
            cand_ms, _ = ctx.timing_read_main()
            launch_ms, launches = ctx.timing_read()
            # the update alone on the last launch (the distribution moves on with every call): wall time, and its kernels' under the context's timer
            tu = []
            ctx.timing_reset()
            for _ in range(steps):
                t0 = time.perf_counter(); ctx.cma_update_batched(E, prm); tu.append((time.perf_counter() - t0) * 1e3)
            first_ms, _ = ctx.timing_read_main()
            all_ms, calls = ctx.timing_read()
            med = lambda k: [r[k]["median"] for r in per_round]
            rec[variant] = {"rounds": per_round, "sigma": [float(x) for x in last["sigma"]], "restarted": [int(x) for x in last["restarted"]],
                            "ratio_cmaes_over_sampling": [float(b / a) for a, b in zip(med("sampling_ms"), med("cmaes_ms"))],
                            "sampling_spread_between_rounds_ms": float(max(med("sampling_ms")) - min(med("sampling_ms"))),
                            "update_call_ms": stats(tu), "update_kernels_ms": all_ms / max(calls, 1), "update_rank_kernel_ms": first_ms / max(calls, 1),
                            "candidate_kernel_ms": cand_ms / max(launches, 1), "rollout_launch_kernels_ms": launch_ms / max(launches, 1)}
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()
    ctx.close()


GRADIENT_SHAPES = [("QuadrupedFlat", 64, 36, [(1, 64), (4, 64), (8, 64), (16, 64)]),
                   ("Cartpole", 64, 128, [(64, 64), (1, 64)])]


def stats(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}


def sweep_gradient(name, precision, H, shapes, steps, warmup, out, mixed=False):
    from mujoco_mpc_amd.planners import GpuBatchGradientPlanner, GpuGradientPlanner, State
    task = load_task(name)
    m = task.model
    rng = np.random.default_rng(1)
    ctx = capi.Context(task.packed_model(differentiable=bool(int(m.get_number("agent_differentiable", 1)))), task.packed(), 0, precision)
    for E, n in shapes:
        raw, clocks, mocap = initial(task, name, E, rng)
        states = []
        for e in range(E):
            st = State(m)
            mp = None if mocap is None else mocap[e].reshape(-1, 7)
            st.set(raw[e][:m.nq], raw[e][m.nq:], mocap_pos=None if mp is None else mp[:, :3], mocap_quat=None if mp is None else mp[:, 3:],
                   time=float(clocks[e]))
            states.append(st)
        singles = [GpuGradientPlanner(precision=precision, backend_factory=lambda t: ctx) for _ in range(E)]
        batch = GpuBatchGradientPlanner(E, precision=precision, backend_factory=lambda t: ctx)
        tasks = mixed_tasks(task, E) if mixed else [task] * E
        for p, t in zip(singles + [batch], tasks + [task]):
            p.initialize(m, t)
            p.num_trajectory = n
            p.allocate()
            p.reset(H)
        if mixed:
            batch.set_tasks(tasks)

        def sequential():
            for p, st in zip(singles, states):
                p.set_state(st)
                p.optimize_policy(H)

        def batched():
            batch.set_states(states)
            batch.optimize_policy(H)

        for _ in range(warmup):
            sequential()
            batched()
        ts, tb, stages = [], [], {}
        for _ in range(steps):   # alternating: both sides see the same clocks and the same neighbours on the machine
            t0 = time.perf_counter(); sequential(); t1 = time.perf_counter(); batched(); t2 = time.perf_counter()
            ts.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
            for k, v in batch.timers.items():
                stages.setdefault(k, []).append(v * 1e-3)
        rec = {"planner": "gradient", "task": name, "precision": precision, "horizon": H, "num_envs": E, "n_per_env": n, "steps": steps,
               "warmup": warmup, "mixed_params": bool(mixed), "kernel": ctx.kernel_name.split(" (")[0], "sequential_ms": stats(ts), "batched_ms": stats(tb),
               "ratio_sequential_over_batched": float(np.median(ts) / np.median(tb)), "beyond_spread": bool(np.max(tb) < np.min(ts)),
               "batched_stage_ms": {k: float(np.median(v)) for k, v in stages.items()},
               "sequential_stage_ms_per_env": {k: float(v) * 1e-3 for k, v in singles[0].timers.items()}}
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()
    ctx.close()


ROBUST_SHAPES = [("QuadrupedFlat", 64, 100, [(1, 2048), (4, 2048), (8, 2048)]),
                 ("Cartpole", 64, 128, [(64, 64)])]


def sweep_robust(name, precision, H, shapes, steps, warmup, out, k, R, mixed=False):
    from mujoco_mpc_amd.planners import GpuBatchRobustPlanner, GpuRobustPlanner, GpuSamplingPlanner, State
    task = load_task(name)
    m = task.model
    rng = np.random.default_rng(1)
    source = capi.Context(task.packed_model(), task.packed(), 0, precision)     # the delegates' rollouts
    ctx = capi.Context(task.packed_model(), task.packed(), 0, precision)        # the perturbed ones
    for E, n in shapes:
        raw, clocks, mocap = initial(task, name, E, rng)
        states = []
        for e in range(E):
            st = State(m)
            mp = None if mocap is None else mocap[e].reshape(-1, 7)
            st.set(raw[e][:m.nq], raw[e][m.nq:], mocap_pos=None if mp is None else mp[:, :3], mocap_quat=None if mp is None else mp[:, 3:],
                   time=float(clocks[e]))
            states.append(st)
        singles = [GpuRobustPlanner(GpuSamplingPlanner(precision=precision, seed=7 + e, backend_factory=lambda t: source), precision=precision,
                                    seed=7 + e, backend_factory=lambda t: ctx) for e in range(E)]
        both = iter([source, ctx])                                               # the fleet allocates its delegate's context first
        batch = GpuBatchRobustPlanner(E, precision=precision, seed=7, backend_factory=lambda t: next(both))
        tasks = mixed_tasks(task, E) if mixed else [task] * E
        for p, t in zip(singles + [batch], tasks + [task]):
            p.initialize(m, t)
            p.ncandidates_, p.nrepetitions_ = k, R
            p.delegate.num_trajectory_ = n
            p.allocate()
            p.reset(H)
        if mixed:
            batch.set_tasks(tasks)

        def sequential():
            for p, st in zip(singles, states):
                p.set_state(st)
                p.optimize_policy(H)

        def batched():
            batch.set_states(states)
            batch.optimize_policy(H)

        for _ in range(warmup):
            sequential()
            batched()
        ts, tb = [], []
        for _ in range(steps):   # alternating: both sides see the same clocks and the same neighbours on the machine
            t0 = time.perf_counter(); sequential(); t1 = time.perf_counter(); batched(); t2 = time.perf_counter()
            ts.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
        rec = {"planner": "robust", "task": name, "precision": precision, "horizon": H, "num_envs": E, "n_per_env": n, "num_candidates": k,
               "repetitions": R, "steps": steps, "warmup": warmup, "mixed_params": bool(mixed), "context_kernel": source.kernel_name.split(" (")[0],
               "note": "context_kernel is the kernel the two contexts were created for: the delegates' rollouts run on it in a launch that reaches "
                       "its threshold (the A1's quad kernel: MJPCX_QUAD_MIN_N candidates in the launch, 2048 by default -- one robot's 2048 "
                       "and a fleet's E x 2048 alike), on the wavefront-per-candidate kernel below it; the perturbed rollouts carry force noise and "
                       "always run on the wavefront-per-candidate kernel (the lane kernels have a NOISY form of their own)",
               "sequential_ms": stats(ts), "batched_ms": stats(tb), "ratio_sequential_over_batched": float(np.median(ts) / np.median(tb)),
               "beyond_spread": bool(np.max(tb) < np.min(ts)), "batched_inside_sequential_range": bool(np.min(ts) <= np.median(tb) <= np.max(ts)),
               "same_choice": bool(all(b.best_candidate == p.best_candidate for b, p in zip(batch.envs, singles)))}
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()
    source.close()
    ctx.close()


SAMPLE_GRADIENT_SHAPES = [("QuadrupedFlat", 64, 100, [(1, 2048), (8, 2048), (16, 2048)])]


def sweep_sample_gradient(name, precision, H, shapes, steps, warmup, out, G, mixed=False):
    from mujoco_mpc_amd.planners import GpuBatchSampleGradientPlanner, GpuSampleGradientPlanner, State
    task = load_task(name)
    m = task.model
    rng = np.random.default_rng(1)
    for E, n in shapes:
        raw, clocks, mocap = initial(task, name, E, rng)
        states = []
        for e in range(E):
            st = State(m)
            mp = None if mocap is None else mocap[e].reshape(-1, 7)
            st.set(raw[e][:m.nq], raw[e][m.nq:], mocap_pos=None if mp is None else mp[:, :3], mocap_quat=None if mp is None else mp[:, 3:],
                   time=float(clocks[e]))
            states.append(st)
        singles = [GpuSampleGradientPlanner(precision=precision, seed=7 + e) for e in range(E)]
        batch = GpuBatchSampleGradientPlanner(E, precision=precision, seed=7)
        tasks = mixed_tasks(task, E) if mixed else [task] * E
        for p, t in zip(singles + [batch], tasks + [task]):
            p.initialize(m, t)
            p.num_trajectory_, p.num_gradient_ = n, G
            p.allocate()
            p.reset(H)
        if mixed:
            batch.set_tasks(tasks)

        def sequential():
            for p, st in zip(singles, states):
                p.set_state(st)
                p.optimize_policy(H)

        def batched():
            batch.set_states(states)
            batch.optimize_policy(H)

        for _ in range(warmup):
            sequential()
            batched()
        ts, tb = [], []
        for _ in range(steps):   # alternating: both sides see the same clocks and the same neighbours on the machine
            t0 = time.perf_counter(); sequential(); t1 = time.perf_counter(); batched(); t2 = time.perf_counter()
            ts.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
        same = bool(all((b.winner, b.winner_type_) == (p.winner, p.winner_type_) and np.array_equal(b.gradient, p.gradient) for b, p in zip(batch.envs, singles)))
        # the batched step in two: the rollout call up to its sync, then the update call alone (the fleet planner's own calls, on its context)
        ctx = batch.ctx
        plans = [batch._resample(p, H) for p in batch.envs]
        times, nominal = np.stack([pl.times() for pl in plans]), np.stack([pl.values() for pl in plans])
        tr, tu = [], []
        for i in range(steps):
            t0 = time.perf_counter()
            batch._push_states()
            ctx.rollout_sample_gradient_batched(n, G, H, batch.interpolation_, times, nominal, batch.noise_exploration, seed=7, iteration=1000 + i, num_envs=E)
            ctx.sync()
            t1 = time.perf_counter()
            ctx.sample_gradient_update_batched(E, G, 0, batch.gradient_filter_, batch.gradient_max_step_size, batch.gradient_min_step_size, batch.noise_exploration)
            t2 = time.perf_counter()
            tr.append((t1 - t0) * 1e3)
            tu.append((t2 - t1) * 1e3)
        rec = {"planner": "sample_gradient", "task": name, "precision": precision, "horizon": H, "num_envs": E, "n_per_env": n, "num_gradient": G,
               "steps": steps, "warmup": warmup, "mixed_params": bool(mixed), "context_kernel": ctx.kernel_name.split(" (")[0],
               "sequential_ms": stats(ts), "batched_ms": stats(tb), "ratio_sequential_over_batched": float(np.median(ts) / np.median(tb)),
               "beyond_spread": bool(np.max(tb) < np.min(ts)), "batched_inside_sequential_range": bool(np.min(ts) <= np.median(tb) <= np.max(ts)),
               "batched_rollout_ms": stats(tr), "batched_update_ms": stats(tu), "same_choice": same}
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()
        for p in singles + [batch]:
            p.ctx.close()


ILQG_SHAPES = [("QuadrupedFlat", 64, 36, [(1, 10), (2, 10), (4, 10), (8, 10), (16, 10)])]


def sweep_ilqg(name, precision, H, shapes, steps, warmup, out, device_chain=None, mixed=False):
    from mujoco_mpc_amd.planners import GpuBatchILQGPlanner, GpuILQGPlanner, State
    task = load_task(name)
    m = task.model
    rng = np.random.default_rng(1)
    ctx = capi.Context(task.packed_model(differentiable=bool(int(m.get_number("agent_differentiable", 1)))), task.packed(), 0, precision)
    for E, n in shapes:
        raw, clocks, mocap = initial(task, name, E, rng)
        states = []
        for e in range(E):
            st = State(m)
            mp = None if mocap is None else mocap[e].reshape(-1, 7)
            st.set(raw[e][:m.nq], raw[e][m.nq:], mocap_pos=None if mp is None else mp[:, :3], mocap_quat=None if mp is None else mp[:, 3:],
                   time=float(clocks[e]))
            states.append(st)
        singles = [GpuILQGPlanner(precision=precision, backend_factory=lambda t: ctx) for _ in range(E)]
        batch = GpuBatchILQGPlanner(E, precision=precision, backend_factory=lambda t: ctx)
        batch.device_chain = device_chain
        tasks = mixed_tasks(task, E) if mixed else [task] * E
        for p, t in zip(singles + [batch], tasks + [task]):
            p.initialize(m, t)
            p.num_rollouts_gui_ = n
            p.allocate()
            p.reset(H)
        if mixed:
            batch.set_tasks(tasks)

        def sequential():
            for p, st in zip(singles, states):
                p.set_state(st)
                p.optimize_policy(H)

        def batched():
            batch.set_states(states)
            batch.optimize_policy(H)

        for _ in range(warmup):
            sequential()
            batched()
        ts, tb, stages = [], [], {}
        for _ in range(steps):   # alternating: both sides see the same clocks and the same neighbours on the machine
            t0 = time.perf_counter(); sequential(); t1 = time.perf_counter(); batched(); t2 = time.perf_counter()
            ts.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
            for k, v in batch.timers.items():
                stages.setdefault(k, []).append(v * 1e-3)
        rec = {"planner": "ilqg", "task": name, "precision": precision, "horizon": H, "num_envs": E, "n_per_env": n, "steps": steps,
               "warmup": warmup, "mixed_params": bool(mixed), "kernel": ctx.kernel_name.split(" (")[0], "sequential_ms": stats(ts), "batched_ms": stats(tb),
               "ratio_sequential_over_batched": float(np.median(ts) / np.median(tb)), "beyond_spread": bool(np.max(tb) < np.min(ts)),
               "device_chain": bool(batch.used_device_chain),
               "batched_stage_ms": {k: float(np.median(v)) for k, v in stages.items()},
               "batched_stage_spread_ms": {k: stats(v) for k, v in stages.items()},
               "sequential_stage_ms_per_env": {k: float(v) * 1e-3 for k, v in singles[0].timers.items()},
               "sat_out": int(sum(batch.sat_out)) if hasattr(batch, "sat_out") else 0}
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()
    ctx.close()


ILQS_SHAPES = [("QuadrupedFlat", 64, 36, [(1, 64), (8, 64), (16, 64)])]
ILQS_ROLLOUTS = 10


def sweep_ilqs(name, precision, H, shapes, steps, warmup, out, device_chain=None):
    from mujoco_mpc_amd.planners import GpuBatchILQSPlanner, GpuILQSPlanner, State
    task = load_task(name)
    m = task.model
    rng = np.random.default_rng(1)
    pm = task.packed_model(differentiable=bool(int(m.get_number("agent_differentiable", 1))))
    ctxs = {"sampling": capi.Context(pm, task.packed(), 0, precision), "ilqg": capi.Context(pm, task.packed(), 0, precision)}

    class Halves:
        """GpuILQSPlanner asks its factory twice, for the sampling half first"""
        def __init__(self):
            self.order = iter(("sampling", "ilqg"))

        def __call__(self, t):
            return ctxs[next(self.order)]

    for E, n in shapes:
        raw, clocks, mocap = initial(task, name, E, rng)
        states = []
        for e in range(E):
            st = State(m)
            mp = None if mocap is None else mocap[e].reshape(-1, 7)
            st.set(raw[e][:m.nq], raw[e][m.nq:], mocap_pos=None if mp is None else mp[:, :3], mocap_quat=None if mp is None else mp[:, 3:],
                   time=float(clocks[e]))
            states.append(st)
        singles = [GpuILQSPlanner(precision=precision, seed=e, backend_factory=Halves()) for e in range(E)]
        fleets = {"batched": GpuBatchILQSPlanner(E, precision=precision, backend_factory=lambda t, half: ctxs[half])}
        fleets["batched"].device_chain = device_chain
        if device_chain is None:
            fleets["batched_no_chain"] = GpuBatchILQSPlanner(E, precision=precision, backend_factory=lambda t, half: ctxs[half])
            fleets["batched_no_chain"].device_chain = False
        for p in singles + list(fleets.values()):
            p.initialize(m, task)
            p.sampling.num_trajectory_ = n
            p.ilqg.num_rollouts_gui_ = ILQS_ROLLOUTS
            p.allocate()
            p.reset(H)

        def sequential():
            for p, st in zip(singles, states):
                p.set_state(st)
                p.optimize_policy(H)

        def batched(p):
            p.set_states(states)
            p.optimize_policy(H)

        for _ in range(warmup):
            sequential()
            for p in fleets.values():
                batched(p)
        times = {k: [] for k in ["sequential"] + list(fleets)}
        stages = {k: {} for k in fleets}
        phases = {k: [] for k in fleets}
        for _ in range(steps):   # alternating: every side sees the same clocks and the same neighbours on the machine
            t0 = time.perf_counter(); sequential(); times["sequential"].append((time.perf_counter() - t0) * 1e3)
            for k, p in fleets.items():
                t0 = time.perf_counter(); batched(p); times[k].append((time.perf_counter() - t0) * 1e3)
                for key, v in p.timers.items():
                    stages[k].setdefault(key, []).append(v * 1e-3)
                step = p.last_step
                phases[k].append({"ms": times[k][-1], "derivatives_backward_ms": p.timers.get("derivatives_backward", 0.0) * 1e-3,
                                  "nominal_phase": int(sum(a == p.ILQG for a in p.previous_active_policy)), "ilqg_ran": int(sum(p.ilqg_ran)),
                                  "from_sampling": None if step is None else int(sum(f == 1 and c >= 0 for f, c in zip(step[0], step[1]))),
                                  "from_ilqg": None if step is None else int(sum(f == 0 and c >= 0 for f, c in zip(step[0], step[1])))})
        rec = {"planner": "ilqs", "task": name, "precision": precision, "horizon": H, "num_envs": E, "n_per_env": n, "ilqg_rollouts": ILQS_ROLLOUTS,
               "steps": steps, "warmup": warmup, "kernel": ctxs["sampling"].kernel_name.split(" (")[0],
               "sequential_ms": stats(times["sequential"]),
               "sequential_active_ilqg": int(sum(p.active_policy == p.ILQG for p in singles))}
        for k, p in fleets.items():
            rec[k + "_ms"] = stats(times[k])
            rec[k + "_device_chain"] = bool(p.used_device_chain)
            rec["ratio_sequential_over_" + k] = float(np.median(times["sequential"]) / np.median(times[k]))
            rec[k + "_stage_ms"] = {key: float(np.median(v)) for key, v in stages[k].items()}
            rec[k + "_stage_spread_ms"] = {key: stats(v) for key, v in stages[k].items()}
            rec[k + "_phases"] = phases[k]
        if "batched_no_chain" in fleets:
            rec["ratio_no_chain_over_chain"] = float(np.median(times["batched_no_chain"]) / np.median(times["batched"]))
            rec["chain_beyond_spread"] = bool(np.max(times["batched"]) < np.min(times["batched_no_chain"]))
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()
    for c in ctxs.values():
        c.close()


def sweep(name, precision, H, shapes, steps, warmup, out, planner="sampling", mixed=False, models=False, prune=False, park=True):
    task = load_task(name)
    m = task.model
    rng = np.random.default_rng(1)
    ctx = capi.Context(task.packed_model(), task.packed(), 0, precision)
    P = int(m.get_number("sampling_spline_points", 6))
    interp = int(m.get_number("sampling_representation", capi.SPLINE_CUBIC))
    std = float(m.get_number("sampling_exploration", 0.1))
    dt = m.get_number("agent_timestep", m.timestep)
    times1 = np.arange(P) * ((H - 1) * dt / max(P - 1, 1))
    for E, n in shapes:
        states, clocks, mocap = initial(task, name, E, rng)
        times, nominal = np.stack([times1] * E), np.zeros((E, P, m.nu))
        it = [0]
        tasks = mixed_tasks(task, E) if mixed else None
        rows = task_rows(tasks) if mixed else None
        # --mixed-models: the fleet's context is given the E models (timed: a setup call); the sequential side plans on E contexts, each created on its model
        set_models_ms, ctxs = None, [ctx] * E
        if models:
            packed = mixed_models(task, E)
            t0 = time.perf_counter()
            ctx.set_models_batched(packed)
            set_models_ms = (time.perf_counter() - t0) * 1e3
            ctxs = [capi.Context(pm, task.packed(), 0, precision) for pm in packed]
        fleet_ctx = ctx

        def plain_params(e):
            if mixed:
                ctxs[e].set_task_params(tasks[e].weight, tasks[e].norm_parameter, tasks[e].parameters or None, tasks[e].risk)

        def fleet_states():
            ctx.set_states(states, clocks, mocap)
            if mixed:
                ctx.set_task_params_batched(**rows)

        def sequential():
            it[0] += 1
            for e in range(E):
                plain_params(e)
                ctx = ctxs[e]
                ctx.set_state(states[e], clocks[e], None if mocap is None else mocap[e])
                ctx.rollout_noise(n, H, interp, times[e], nominal[e], capi.make_noise_spec(seed=7 + e, iteration=it[0], std0=std))
                ctx.best(0)

        # --prune: the batched side retires and parks per environment (set_pruning_batched), as GpuBatchSamplingPlanner(pruning=True) does:
        # on for the launch alone, every robot's hint its previous best return x 1.05 (--no-park: no hints)
        last_best, counts = [None], []

        def batched():
            fleet_states()
            if prune:
                hints = None if not park or last_best[0] is None else 1.05 * last_best[0]
                ctx.set_pruning_batched(True, E, None, hints)
            try:
                ctx.rollout_noise_batched(n, H, interp, times, nominal, capi.make_noise_spec(seed=7, iteration=it[0], std0=std), num_envs=E)
            finally:
                if prune:
                    ctx.set_pruning_batched(False)
            if prune:
                counts.append(ctx.prune_stats_batched(E))
            last_best[0] = ctx.best_batched(E, 0)[1]

        ce = planner == "cross_entropy"
        n_elite = max(n // 10, 2)
        variance = np.stack([np.full((P, m.nu), (std * (1 + 0.1 * e)) ** 2) for e in range(E)])   # every robot its own

        def ce_spec(e, row):
            return capi.make_noise_spec(seed=7 + e, iteration=it[0], mode=capi.NOISE_CROSS_ENTROPY, nominal_candidate=n - 1,
                                        explore_count=n // 10, std0=std, std1=0.1 * std, param_variance=row)

        def ce_sequential():   # GpuCrossEntropyPlanner.optimize_policy's calls
            it[0] += 1
            for e in range(E):
                plain_params(e)
                ctx = ctxs[e]
                ctx.set_state(states[e], clocks[e], None if mocap is None else mocap[e])
                ctx.rollout_noise(n, H, interp, times[e], nominal[e], ce_spec(e, variance[e]))
                idx, _ = ctx.topk(n_elite + 1)
                idx = idx[idx != n - 1][:n_elite]
                s, _ = ctx.elite_moments(idx)
                ctx.elite_moments(idx, s / n_elite)

        # --prune: the batched side runs at rank n_elite + 1 (set_prune_rank) with a bound per environment, as
        # GpuBatchCrossEntropyPlanner(pruning=True) does: on for the launch alone, every robot's hint its previous worst elite return x 1.05
        # (--no-park: no hints)
        last_worst = [None]

        def ce_rollout():
            fleet_states()
            if prune:
                ctx.set_prune_rank(n_elite + 1)
                ctx.set_pruning_batched(True, E, None, None if not park or last_worst[0] is None else 1.05 * last_worst[0])
            try:
                ctx.rollout_noise_batched_ce(n, H, interp, times, nominal, variance, ce_spec(0, None), num_envs=E)
            finally:
                if prune:
                    ctx.set_pruning_batched(False)
                    ctx.set_prune_rank(1)
            if prune:
                counts.append(ctx.prune_stats_batched(E))

        def ce_batched():      # GpuBatchCrossEntropyPlanner.optimize_policy's calls
            ce_rollout()
            last_worst[0] = ctx.ce_update_batched(E, n_elite, n - 1)[1][:, n_elite - 1].copy()

        if ce:
            sequential, batched = ce_sequential, ce_batched
        for _ in range(warmup):
            sequential()
            batched()
        ts, tb = [], []
        for _ in range(steps):   # alternating: both sides see the same clocks and the same neighbours on the machine
            t0 = time.perf_counter(); sequential(); t1 = time.perf_counter(); batched(); t2 = time.perf_counter()
            ts.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
        rec = {"task": name, "precision": precision, "horizon": H, "num_envs": E, "n_per_env": n, "steps": steps, "warmup": warmup,
               "mixed_params": bool(mixed), "mixed_models": bool(models), "set_models_ms": set_models_ms, "kernel": ctx.kernel_name.split(" (")[0],
               "sequential_ms": {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))},
               "batched_ms": {"median": float(np.median(tb)), "min": float(np.min(tb)), "max": float(np.max(tb))},
               "ratio_sequential_over_batched": float(np.median(ts) / np.median(tb)),
               "beyond_spread": bool(np.max(tb) < np.min(ts))}
        if prune:   # per environment, summed over the timed steps: how much of the fleet left early, and how
            timed = counts[-steps:]
            rec.update(prune=True, park=bool(park), candidates_per_env=int(n) * steps,
                       **{k: [int(sum(c[k][e] for c in timed)) for e in range(E)] for k in ("retired", "retire_step_sum", "parked", "settled_retired", "resumed")})
        if ce:
            tr, tu = [], []
            for _ in range(steps):
                t0 = time.perf_counter(); ce_rollout(); ctx.sync(); t1 = time.perf_counter()
                last_worst[0] = ctx.ce_update_batched(E, n_elite, n - 1)[1][:, n_elite - 1].copy(); t2 = time.perf_counter()
                tr.append((t1 - t0) * 1e3)
                tu.append((t2 - t1) * 1e3)
            rec.update(planner="cross_entropy", n_elite=n_elite,
                       batched_rollout_ms={"median": float(np.median(tr)), "min": float(np.min(tr)), "max": float(np.max(tr))},
                       batched_update_ms={"median": float(np.median(tu)), "min": float(np.min(tu)), "max": float(np.max(tu))})
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()
        if models:
            for c in ctxs:
                c.close()
    fleet_ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--planner", choices=["sampling", "cross_entropy", "gradient", "ilqg", "ilqs", "robust", "sample_gradient", "ensemble", "mppi", "cmaes"], default="sampling")
    ap.add_argument("--shapes", default=None, help="comma-separated ExN filter, e.g. 8x2048,1x16384")
    ap.add_argument("--mixed-params", action="store_true", help="every environment its own task weights, parameters and risk")
    ap.add_argument("--mixed-models", action="store_true", help="sampling, cross_entropy, ensemble: every environment its own model (payload, friction, actuator strength)")
    ap.add_argument("--tail", type=int, default=None, help="--planner ensemble: the score is the mean of the `tail` largest returns (default: all, the mean)")
    ap.add_argument("--temperature", type=float, default=None, help="--planner mppi: the temperature (default: a tenth of the spread of the first launch's returns)")
    ap.add_argument("--rounds", type=int, default=2, help="--planner mppi, cmaes: rounds of --steps alternating timed steps")
    ap.add_argument("--robust", default="16x4", help="--planner robust: candidates x repetitions")
    ap.add_argument("--gradient-candidates", type=int, default=32, help="--planner sample_gradient: gradient candidates per environment")
    ap.add_argument("--prune", action="store_true", help="--planner sampling, cross_entropy: the batched side prunes and parks per environment (set_pruning_batched; "
                    "cross_entropy: at rank n_elite + 1, set_prune_rank)")
    ap.add_argument("--no-park", action="store_true", help="with --prune: no park hints")
    ap.add_argument("--no-device-chain", action="store_true", help="--planner ilqg, ilqs: the sequential middle (the A/B of ilqg_step_batched[_from])")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", {"cross_entropy": "batch_sweep_ce.jsonl", "gradient": "batch_sweep_gradient.jsonl", "ilqg": "batch_sweep_ilqg.jsonl", "ilqs": "batch_sweep_ilqs.jsonl", "robust": "batch_sweep_robust.jsonl",
                                                       "sample_gradient": "batch_sweep_sample_gradient.jsonl", "ensemble": "batch_sweep_ensemble.jsonl", "mppi": "batch_sweep_mppi.jsonl", "cmaes": "batch_sweep_cmaes.jsonl"}.get(a.planner, "batch_sweep.jsonl"))
    keep = None if a.shapes is None else {tuple(int(x) for x in sh.split("x")) for sh in a.shapes.split(",")}
    if a.steps < 10:
        raise SystemExit("batch_sweep.py: at least 10 timed steps")
    with open(a.out, "w") as out:
        for name, precision, H, shapes in {"gradient": GRADIENT_SHAPES, "ilqg": ILQG_SHAPES, "ilqs": ILQS_SHAPES, "robust": ROBUST_SHAPES,
                                             "sample_gradient": SAMPLE_GRADIENT_SHAPES, "ensemble": ENSEMBLE_SHAPES, "mppi": MPPI_SHAPES, "cmaes": MPPI_SHAPES}.get(a.planner, SHAPES):
            shapes = [sh for sh in shapes if keep is None or sh in keep]
            if keep is not None and a.only == name and a.planner in ("sampling", "cross_entropy"):   # (--only with --shapes: also shapes outside the default list, e.g. 16x1024)
                shapes += [sh for sh in sorted(keep) if sh not in shapes]
            if shapes and (a.only is None or a.only == name):
                if a.planner == "ensemble":
                    sweep_ensemble(name, precision, H, shapes, a.steps, a.warmup, out, a.tail, a.mixed_models)
                    continue
                if a.planner == "mppi":
                    sweep_mppi(name, precision, H, shapes, a.steps, a.warmup, out, a.temperature, a.rounds)
                    continue
                if a.planner == "cmaes":
                    sweep_cmaes(name, precision, H, shapes, a.steps, a.warmup, out, a.rounds)
                    continue
                if a.mixed_models and (a.planner not in ("sampling", "cross_entropy") or name == "Cartpole"):
                    if a.planner not in ("sampling", "cross_entropy"):
                        raise SystemExit("batch_sweep.py: --mixed-models is for --planner sampling and cross_entropy")
                    continue      # (a lane-family task: its model constants are fixed when the library is built)
                if a.planner == "gradient":
                    sweep_gradient(name, precision, H, shapes, a.steps, a.warmup, out, a.mixed_params)
                elif a.planner == "robust":
                    k, R = (int(x) for x in a.robust.split("x"))
                    sweep_robust(name, precision, H, shapes, a.steps, a.warmup, out, k, R, a.mixed_params)
                elif a.planner == "sample_gradient":
                    sweep_sample_gradient(name, precision, H, shapes, a.steps, a.warmup, out, a.gradient_candidates, a.mixed_params)
                elif a.planner == "ilqs":
                    if a.mixed_params:
                        raise SystemExit("batch_sweep.py: --planner ilqs has no --mixed-params")
                    sweep_ilqs(name, precision, H, shapes, a.steps, a.warmup, out, False if a.no_device_chain else None)
                elif a.planner == "ilqg":
                    sweep_ilqg(name, precision, H, shapes, a.steps, a.warmup, out, False if a.no_device_chain else None, a.mixed_params)
                else:
                    if a.prune and a.planner not in ("sampling", "cross_entropy"):
                        raise SystemExit("batch_sweep.py: --prune is for --planner sampling and --planner cross_entropy")
                    sweep(name, precision, H, shapes, a.steps, a.warmup, out, a.planner, a.mixed_params, a.mixed_models, a.prune, not a.no_park)


if __name__ == "__main__":
    main()
