#!/usr/bin/env python3
"""K launches of the north-star batch (QuadrupedFlat, Predictive-Sampling noise, 16384 x 100, fp64) and nothing else: the rocprofv3 target
for the quad kernel (kernel trace, PMC passes)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# python tools/quad_prof.py --stamps LOG: the sub-stamps of a QEXP_SUBSTAMPS build (quad_kernel.h; slots 46..63 of the "raw counters 40..63"
# lines an MJPCX_QUAD_STAMPS=1 run prints) with their names, per launch: cycles of wavefront 0 over the launch's steps, counts per launch
SUB = {46: "floor: centre + axis + pair boxes, orientation", 47: "floor: bounding tests + candidate points", 48: "floor: contact creation",
       49: "#floor: contact-creation trips", 50: "pairs: leg-level cull", 51: "pairs: hand-over + call", 52: "pairs: own geoms' boxes",
       53: "pairs: pretests", 54: "#pairs: sources walked", 55: "pairs: partner fetch", 56: "pairs: exact tests", 57: "pairs: other quads' sources (+ return)",
       58: "#pairs: calls of the tests", 59: "#floor: geoms the wavefront skipped"}
if len(sys.argv) > 2 and sys.argv[1] == "--stamps":
    rows = [[int(x) for x in l.split(":")[1].split()] for l in open(sys.argv[2]) if "raw counters 40..63" in l]
    for k, name in sorted(SUB.items()):
        print(f"{k:3d} {name:52s}" + "".join(f"{r[k - 40]:>10d}" for r in rows))
    sys.exit(0)
import numpy as np
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.task import load_task
K = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
t = load_task("QuadrupedFlat"); t.transition(0.0)
pm, pt = t.packed_model(), t.packed()
state = np.concatenate([t.model.keyframes["home"]["qpos"], np.zeros(18)])
mocap = np.array([0.3, 0, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])
H, P = 100, 3
times = np.arange(P) * ((H - 1) * 0.01 / (P - 1))
ctx = capi.Context(pm, pt, 0, 64)
ctx.set_state(state, 0.0, mocap)
ns = capi.make_noise_spec(seed=11, iteration=3, mode=capi.NOISE_SAMPLING, std0=0.04)
for k in range(K):
    ctx.rollout_noise(N, H, 0, times, np.zeros((P, 12)), ns)
ctx.sync()
print("done", ctx.kernel_name)
