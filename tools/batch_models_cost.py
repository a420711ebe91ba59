"""What a model per environment costs (mjpcx_set_models_batched). Three measurements, one JSON line per record:

  setup    the call itself, E = 8 and 16, on the A1 (fp64: quad + registered-model images) and the Humanoid (fp32: limb + registered-model
           images): the builders run once per model on the host -- a setup call, not for a plan loop. Median of five calls.
  control  the batched plan step of eight A1s x 2048 candidates, H = 100, on three contexts in turn: no models; eight COPIES of the
           context's own model (the model path alone); eight unlike models (tools/batch_sweep.py's mixed_models: the path and the physics).
  generic  the same three on the generic wavefront-per-candidate kernel (MJPCX_NO_LDS_MODEL=1), eight A1s x 64 candidates, H = 36: that
           kernel reads its model through its kernel arguments and is launched once per environment when models are set -- what a fleet
           on it pays for losing the one launch, at a small share per environment.

python tools/batch_models_cost.py [--only setup|control|generic] [--out profiles/batch_models_cost.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import batch_sweep  # noqa: E402
from mujoco_mpc_amd import capi  # noqa: E402
from mujoco_mpc_amd.task import load_task  # noqa: E402


def stats(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}


def setup(emit):
    for name, precision in (("QuadrupedFlat", 64), ("HumanoidTrack", 32)):
        task = load_task(name)
        task.transition(0.0) if name == "QuadrupedFlat" else task.transition(0.0, mode=9)
        ctx = capi.Context(task.packed_model(), task.packed(), 0, precision)
        for E in (8, 16):
            packed = batch_sweep.mixed_models(task, E)
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                ctx.set_models_batched(packed)
                ts.append((time.perf_counter() - t0) * 1e3)
            emit({"measurement": "setup", "task": name, "precision": precision, "kernel": ctx.kernel_name.split(" (")[0], "num_envs": E,
                  "set_models_batched_ms": stats(ts)})
        ctx.close()


def plan_step(emit, measurement, E, n, H, env, steps=12, warmup=2):
    name, precision = "QuadrupedFlat", 64
    task = load_task(name)
    m = task.model
    P = int(m.get_number("sampling_spline_points", 6))
    interp = int(m.get_number("sampling_representation", capi.SPLINE_CUBIC))
    std = float(m.get_number("sampling_exploration", 0.1))
    dt = m.get_number("agent_timestep", m.timestep)
    times, nominal = np.stack([np.arange(P) * ((H - 1) * dt / max(P - 1, 1))] * E), np.zeros((E, P, m.nu))
    states, clocks, mocap = batch_sweep.initial(task, name, E, np.random.default_rng(1))
    unlike = batch_sweep.mixed_models(task, E)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctxs = {kind: capi.Context(task.packed_model(), task.packed(), 0, precision) for kind in ("none", "copies", "unlike")}
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    for kind, c in ctxs.items():
        if kind != "none":
            c.set_models_batched([unlike[0]] * E if kind == "copies" else unlike)
    ts = {k: [] for k in ctxs}
    for r in range(warmup + steps):   # alternating: the three see the same clocks and the same neighbours on the machine
        for kind, c in ctxs.items():
            t0 = time.perf_counter()
            c.set_states(states, clocks, mocap)
            c.rollout_noise_batched(n, H, interp, times, nominal, capi.make_noise_spec(seed=7, iteration=r + 1, std0=std), num_envs=E)
            c.best_batched(E, 0)
            if r >= warmup:
                ts[kind].append((time.perf_counter() - t0) * 1e3)
    for kind, c in ctxs.items():
        emit({"measurement": measurement, "task": name, "precision": precision, "kernel": c.kernel_name.split(" (")[0], "num_envs": E, "n_per_env": n,
              "horizon": H, "steps": steps, "models": kind, "batched_ms": stats(ts[kind])})
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["setup", "control", "generic"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_models_cost.jsonl"))
    a = ap.parse_args()
    with open(a.out, "w") as out:
        def emit(rec):
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
            out.flush()
        if a.only in (None, "setup"):
            setup(emit)
        if a.only in (None, "control"):
            plan_step(emit, "control", 8, 2048, 100, {})
        if a.only in (None, "generic"):
            plan_step(emit, "generic", 8, 64, 36, {"MJPCX_NO_LDS_MODEL": "1"})


if __name__ == "__main__":
    main()
