#!/usr/bin/env python3
"""How much of a Predictive-Sampling launch pruning can retire, from the CPU oracle alone (no GPU): the bench's loop -- QuadrupedFlat, home
keyframe, sigma 0.04, 3 zero-order-hold nodes, H = 100, the winner becoming the next nominal -- with the per-step costs of every candidate.
    python tools/prune_probe.py [N = 4096] [iterations = 14] [threads = 16]
Per plan iteration: the spread of the returns, and with the launch's FINAL best as the bound (the most pruning could do; in a launch the
bound only becomes available when the first wavefronts finish) the share of candidates whose partial return exceeds it by step 60 .. 90,
the mean retire step, and the step at which a wavefront of 16 consecutive candidates has lost all of them (its exit step)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mujoco_mpc_amd import capi  # noqa: E402
from mujoco_mpc_amd.task import load_task  # noqa: E402
from oracle import pyoracle  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
ITER = int(sys.argv[2]) if len(sys.argv) > 2 else 14
THREADS = int(sys.argv[3]) if len(sys.argv) > 3 else 16
H, P, SIGMA = 100, 3, 0.04
MOCAP = np.array([0.3, 0, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])

task = load_task("QuadrupedFlat")
task.transition(0.0)
pm, pt = task.packed_model(), task.packed()
state = np.concatenate([task.model.keyframes["home"]["qpos"], np.zeros(18)])
times = np.arange(P) * ((H - 1) * 0.01 / P)
nominal = np.zeros((P, 12))
for it in range(ITER):
    ns = capi.make_noise_spec(seed=0, iteration=it, mode=capi.NOISE_SAMPLING, std0=SIGMA)
    nodes = pyoracle.noise_candidates(pm, ns, P, nominal, np.arange(N))
    out = pyoracle.rollout_batch(pm, pt, state, 0.0, MOCAP, N, H, P, capi.SPLINE_ZERO, times, nodes, num_threads=THREADS)
    ret, costs = out["total_return"], out["costs"]
    assert costs.min() >= 0
    best = ret.min()
    partial = np.cumsum(costs, axis=1) / H
    over = partial[:, :H - 1] > best
    over[0] = False  # the nominal is never retired
    retire = np.where(over.any(axis=1), over.argmax(axis=1), H - 1)
    by = " ".join(f"by {s}: {100 * np.mean(retire <= s):.0f} %" for s in (60, 70, 80, 90))
    waves = retire[:N - N % 16].reshape(-1, 16).max(axis=1)
    print(f"iteration {it:2d}: best {best:.4f} median {np.median(ret):.3f} p99 {np.quantile(ret, 0.99):.3f} | retired {by}; never {100 * np.mean(retire == H - 1):.2f} %; "
          f"mean retire step {retire[retire < H - 1].mean():.1f}; wavefront exit step mean {waves.mean():.1f}", flush=True)
    nominal = nodes[int(ret.argmin())]
