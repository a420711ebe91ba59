"""-m gpu: the task residuals of every rollout kernel against answers known before any kernel runs (tests/residual_cases.py: an independent
mpmath reference built on forward kinematics by homogeneous transforms, velocities by differentiating positions, closed-form ground heights
and the tasks' design constants; anchor cases with hand-derived literals).

Each row is one kernel, forced with the switches of tests/test_gpu_step_parity.py::ROWS and asserted on its kernel name before and after. One
context per row; each case moves in with set_state, set_residual_state and set_task_params, rolls out ONE step (horizon 2, one zero-order
node, three candidates: zero control, a random control, a control past the range) and residual[:, 0, :] is compared with the expected row
(only the control entries differ between the candidates), trace[:, 0] with the reference's head site (A1).

Bounds: fp64 rows |d - e| <= 1e-9 (1 + |e|), the project's one-step fp64 bound; fp32 rows the standing per-step goal STEP_GOAL = 1e-4 on
|d - e| / (1 + |e|), e evaluated at the float32-rounded state, time, mocap, frozen reals and parameters. fp32 rows leave out the cases on a
comparison a float kernel makes at another threshold (`fp64_only`: the flip's four phase instants, |angvel| = 0.01) and the cases whose expected
row moves by more than a tenth of the goal when one input moves by one float32 ulp (residual_cases.FP32_EXCLUDED: gait/Walk/amplitude0, an
amplitude of exactly 0, and humanoid/clip3/t1.250, a time exactly on a key); the fp64 rows leave out none.

    row                          kernel                          cases   worst measured on MI355X        at
    quad-fp64                    rollout_quad_kernel             46      8.4e-16                         terrain/hill, Gait
    tree-a1-fp64                 rollout_tree_kernel<A1>         46      9.5e-16                         terrain/inside-box, Balance
    tree-a1-fp32                 rollout_tree_kernel<A1>         40      1.3e-06                         terrain/hill, Balance
    wave-rk4-a1-fp64             rollout_wave_kernel             46      9.5e-16                         terrain/inside-box, Balance
    wave-rk4-a1-fp32             rollout_wave_kernel             40      1.3e-06                         terrain/hill, Balance
    limb-fp64                    rollout_limb_kernel             14      2.0e-15                         humanoid/clip9/t16.957
    limb-fp32                    rollout_limb_kernel             13      4.5e-06                         humanoid/clip3/t0.500
    tree-humanoid-fp64           rollout_tree_kernel<Humanoid>   14      1.4e-15                         humanoid/clip9/t16.957
    tree-humanoid-fp32           rollout_tree_kernel<Humanoid>   13      4.5e-06                         humanoid/clip3/t0.500
    wave-rk4-humanoid-fp64       rollout_wave_kernel             14      1.4e-15                         humanoid/clip9/t16.957
    lane-cartpole-fp64 / fp32    rollout_lane                    6       5.0e-17 / 3.4e-08
    lane-particle-fp64 / fp32    rollout_lane                    3       0 / 1.0e-08
    lane-particlecopy-fp64/fp32  rollout_lane                    3       0 / 0

The sixteen rows take 1.2 s on the device together (0.9 s of it the quad context); the module adds about 4 s to the -m gpu suite, half of it
the 72 cases' expected rows in 50-digit arithmetic (shared with tests/test_residual_cases.py when both run in one session).

What the first run found: under RK4 the wavefront and lane kernels, and the oracle with them, recorded the trace of a step from the LAST
stage's site positions (2.6e-2 off the head site on quadruped/tumbling0). The trace is a framepos sensor and the stages after the first
run no sensor stage, so it is the position the step starts from, as under Euler; every copy now records that.

On the rows of rollout_quad_kernel and rollout_limb_kernel the candidates the kernel hands on to the wavefront kernels are counted: the
branch census must be complete over the cases it kept every candidate of."""
import time

import numpy as np
import pytest

import residual_cases as rc
import test_gpu_step_parity as sp

pytestmark = pytest.mark.gpu

A1, HUM = "QuadrupedFlat", "HumanoidTrack"
# id: (task, the row of test_gpu_step_parity.ROWS whose switches and kernel name it takes, precision, integrator (None: the task's))
ROWS = {
    "quad-fp64": (A1, "quad-fp64", 64, None),
    "tree-a1-fp64": (A1, "tree-a1-fp64", 64, None),
    "tree-a1-fp32": (A1, "tree-a1-fp32", 32, None),
    "wave-rk4-a1-fp64": (A1, "wave-rk4-a1-fp64", 64, 1),
    "wave-rk4-a1-fp32": (A1, "wave-rk4-a1-fp32", 32, 1),
    "limb-fp64": (HUM, "limb-fp64", 64, None),
    "limb-fp32": (HUM, "limb-fp32", 32, None),
    "tree-humanoid-fp64": (HUM, "tree-humanoid-fp64", 64, None),
    "tree-humanoid-fp32": (HUM, "tree-humanoid-fp32", 32, None),
    "wave-rk4-humanoid-fp64": (HUM, "wave-rk4-humanoid-fp64", 64, 1),
    "lane-cartpole-fp64": ("Cartpole", "lane-cartpole-fp64", 64, None),
    "lane-cartpole-fp32": ("Cartpole", "lane-cartpole-fp32", 32, None),
    "lane-particle-fp64": ("Particle", "lane-particle-fp64", 64, None),
    "lane-particle-fp32": ("Particle", "lane-particle-fp32", 32, None),
    "lane-particlecopy-fp64": ("ParticleCopy", "lane-particle-fp64", 64, None),
    "lane-particlecopy-fp32": ("ParticleCopy", "lane-particle-fp32", 32, None),
}
TASK_BRANCHES = {A1: frozenset(b for b in rc.BRANCHES if not b.startswith("humanoid:")),
                 HUM: frozenset(b for b in rc.BRANCHES if b.startswith("humanoid:"))}
FP64_ONLY_BRANCHES = frozenset(["walk:threshold", "step-zero:amplitude"])   # (the branches only the cases an fp32 row leaves out reach)


def controls(c, k):
    a = rc.task_of(c.task).model.arrays
    lo, hi = a["actuator_ctrlrange"][:, 0], a["actuator_ctrlrange"][:, 1]
    rng = np.random.default_rng(500 + k)
    return np.stack([np.zeros(len(lo)), rng.uniform(lo, hi), np.asarray(c.ctrl, float)])[:, None, :]   # (the case's own control reaches past the range)


@pytest.mark.parametrize("row", list(ROWS))
def test_residual_row_against_the_reference(row):
    task, parity_row, precision, integrator = ROWS[row]
    _, env, kernel, _, _, _, _ = sp.ROWS[parity_row]
    single = precision == 32
    bound = rc.STEP_GOAL if single else rc.FP64_BOUND
    left_out = rc.FP32_EXCLUDED if single else frozenset()
    todo = [c for c in rc.cases(task) if not (single and (c.fp64_only or c.name in left_out))]
    assert 10 * len(left_out & {c.name for c in rc.cases(task)}) <= len(rc.cases(task))
    t = rc.task_of(task)
    pm = t.packed_model()
    if integrator is not None:
        pm.struct.integrator = integrator
    began = time.perf_counter()
    ctx = sp.context(pm, t.packed(), precision, env)
    worst, where, missed, kept_labels, handed = 0.0, "", [], set(), 0
    try:
        assert ctx.kernel_name.startswith(kernel), ctx.kernel_name
        for k, c in enumerate(todo):
            nodes = controls(c, k)
            ctx.set_state(c.state, c.time, c.mocap)
            if c.residual_int or c.residual_real:
                ctx.set_residual_state(c.residual_int, c.residual_real)
            if c.parameters:
                ctx.set_task_params(parameters=c.parameters, risk=t.risk)
            ctx.rollout_splines(2, 0, np.array([c.time]), nodes)
            ctx.returns()
            on = ctx.quad_stats()["handed_on"] if kernel in ("rollout_quad_kernel", "rollout_limb_kernel") else 0
            handed += on
            if not on:
                kept_labels |= c.labels
            for cand in range(len(nodes)):
                tr = ctx.fetch_trajectory(cand)
                e = rc.expected_for(c, nodes[cand, 0], single)
                err = np.abs(tr.residual[0] - e) / (1 + np.abs(e))
                err = np.where(np.isnan(err), np.inf, err)
                if c.head is not None:
                    err = np.concatenate([err, np.abs(tr.trace[0] - c.head) / (1 + np.abs(c.head))])
                i = int(np.argmax(err))
                if err[i] > worst:
                    worst, where = float(err[i]), f"{c.name}, candidate {cand}, entry {i}"
                if not err[i] <= bound:
                    got = tr.residual[0][i] if i < len(e) else tr.trace[0][i - len(e)]
                    missed.append((float(err[i]), f"{c.name}, candidate {cand}, entry {i}: device {got!r}, expected {(e[i] if i < len(e) else c.head[i - len(e)])!r}"))
        assert ctx.kernel_name.startswith(kernel), ctx.kernel_name      # (the moves kept the context on its kernel)
    finally:
        ctx.close()
    print(f"{row}: {kernel}, {len(todo)} cases x 3 candidates, worst {worst:.2e} (bound {bound:.0e}) at {where}; handed on {handed}; "
          f"{time.perf_counter() - began:.2f} s")
    assert not missed, sorted(missed, reverse=True)[:6]
    if task in TASK_BRANCHES:
        want = TASK_BRANCHES[task] - (FP64_ONLY_BRANCHES if single else frozenset())
        assert kept_labels >= want, sorted(want - kept_labels)


@pytest.mark.parametrize("row", ["lane-cartpole-fp64", "lane-cartpole-fp32", "lane-particle-fp64", "lane-particle-fp32"])
def test_the_trace_of_a_lane_step_does_not_depend_on_the_integrator(row):
    """the trace of a step is the framepos sensor at the state the step starts from: the lane kernels record the same trace[:, 0] under RK4 as
    under Euler (before, RK4 recorded the last stage's site positions: the trace one step on, which the states here tell apart)"""
    task, parity_row, precision, _ = ROWS[row]
    _, env, kernel, _, _, _, _ = sp.ROWS[parity_row]
    bound = rc.STEP_GOAL if precision == 32 else rc.FP64_BOUND
    t = rc.task_of(task)
    traces = {}
    for integrator in (0, 1):
        pm = t.packed_model()
        pm.struct.integrator = integrator
        ctx = sp.context(pm, t.packed(), precision, env)
        try:
            assert ctx.kernel_name.startswith(kernel), ctx.kernel_name
            rows = []
            for k, c in enumerate(rc.cases(task)):
                nodes = controls(c, k)
                ctx.set_state(c.state, c.time, c.mocap)
                ctx.rollout_splines(2, 0, np.array([c.time]), nodes)
                ctx.returns()
                rows.append(np.stack([ctx.fetch_trajectory(cand).trace for cand in range(len(nodes))]))
            traces[integrator] = np.stack(rows)          # [case, candidate, step, 3 x traces]
        finally:
            ctx.close()
    first, after = traces[0][:, :, 0], traces[0][:, :, 1]
    assert np.max(np.abs(after - first)) > 1e-3                                   # (the bodies move: one step on is another trace)
    err = np.abs(traces[1][:, :, 0] - first) / (1 + np.abs(first))
    print(f"{row}: trace[:, 0] under RK4 against Euler, worst {err.max():.2e} (bound {bound:.0e})")
    assert err.max() <= bound
