#!/usr/bin/env python3
"""mjpcx_prune_stats and mjpcx_park_stats over the bench's loop (QuadrupedFlat Predictive Sampling, 16384 x 100, fp64, through the C++ planner,
planning again and again from one state): per launch the hint, candidates parked / retired by the settling pass / resumed, all retirements
and their mean step, wavefronts that ended early, the best score; then the means over the 20 timed launches (profiles/r11_park_counters.log):
    python tools/park_counters.py [slack]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from mujoco_mpc_amd.hostplanner import HostPlanner
from mujoco_mpc_amd.task import load_task
task = load_task("QuadrupedFlat")
N, H = 16384, 100
pl = HostPlanner(task, device=0, precision=64, seed=0, num_trajectory=N, kind="sampling")
if len(sys.argv) > 1:
    pl.park_set(float(sys.argv[1]))
qpos, qvel, mp, mq = bench.initial_condition("QuadrupedFlat", task, pl)
pl.reset(H)
pl.set_state(qpos, qvel, 0.0, mocap_pos=mp, mocap_quat=mq)
rows = []
for step in range(26):
    pl.optimize_policy(H)
    s, k = pl.prune_stats(), pl.park_info()
    rows.append(s + [k["parked"], k["settled_retired"], k["resumed"]])
    print(f"launch {step:2d}{' (warm-up)' if step < 6 else ''}: hint {k['hint']:.4f}, parked {k['parked']} ({100 * k['parked'] / N:.1f} %), settled-retired {k['settled_retired']}, "
          f"resumed {k['resumed']}; retired {s[0]} of {N} ({100 * s[0] / N:.1f} %), mean retire step {s[1] / max(s[0], 1):.1f}, negative-cost flag {s[2]}, "
          f"wavefronts ended early {s[3]} of 1024, best {pl.best_score:.4f}")
t = np.array(rows[6:], float)
print(f"timed launches: parked {t[:, 4].mean() / N * 100:.1f} %, settled-retired {t[:, 5].mean() / N * 100:.1f} %, resumed {t[:, 6].mean() / N * 100:.2f} % (max {t[:, 6].max():.0f}); "
      f"retired {t[:, 0].mean() / N * 100:.1f} % (min {t[:, 0].min() / N * 100:.1f}, max {t[:, 0].max() / N * 100:.1f}), mean retire step "
      f"{(t[:, 1] / np.maximum(t[:, 0], 1)).mean():.1f}, wavefronts ended early {t[:, 3].mean():.0f} of 1024 (min {t[:, 3].min():.0f}, max {t[:, 3].max():.0f}); "
      f"steps not rolled out {100 * ((H - 1) * t[:, 0] - t[:, 1]).sum() / (20 * N * (H - 1)):.1f} % of all candidate-steps")
pl.close()
