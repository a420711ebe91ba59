"""-m gpu: norm_value<T, N> (csrc/device_common.h) and lane_cost's risk transform (csrc/rollout_lane.h), the cost every candidate pays at
every step, in fp64 and in fp32, against the exact answers of tests/cost_cases.py.

The Particle's residual is (qpos - goal, qvel). One context per norm type and precision carries the norm under test on term 0 and a
quadratic of small weight on term 1; mjpcx_set_states gives environment e the state and the goal that put its step-0 residual on the
point the test chose, mjpcx_set_task_params_batched gives it its own p, q, weights and risk, and one mjpcx_rollout_splines_batched of
two steps evaluates them all.

   the stored step-0 residual is the intended point: fl(qpos - goal) in the context's precision, exactly
   the step-0 cost of two candidates of an environment is the same bits (step 0 does not depend on the spline)
   that cost is within the derived bound, at u = 2^-53 or 2^-24, of the mpmath value of BaseResidualFn::CostValue (task.cc:71-110) AT
       THE STORED INPUTS: the fp32 context's residual, p, q, weights and risk are the fp32 roundings, and the exact answer is taken there
   points: every point of cost_cases.points() whose value is finite -- the zeros, the signed zeros, |x| from 1e-8 to 1e3, the branch
       points, rectify with p <= 0, and |x| << p for L2, smooth-abs and smooth-abs2, where s - p cancels (the bound carries u p into the
       difference; tests/test_cost_cases.py shows numpy float32 inside a quarter of it) -- under the risks 0, 9e-7, -1.1e-6, +-0.7

The w_norm_* functions of the wave and tree kernels and the per-entry norms of the quad and limb kernels take residuals no test can
inject exactly; they stay with the step-parity tests. Worst error / bound, measured on an MI355X: DESIGN.md 4.3."""
import numpy as np
import pytest

import cost_cases as cc
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.task import load_task

pytestmark = pytest.mark.gpu
N, H, P = 64, 2, 3


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("t", cc.VALUE_NORMS)
def test_step_cost_of_every_point(t, precision):
    cases = cc.value_cases(t, precision)
    E = len(cases)
    assert E >= 10
    task = cc.task_with(load_task("Particle"), cases[0].spec)
    pm = task.packed_model()
    ctx = capi.Context(pm, task.packed(), 0, precision)
    assert "rollout_lane" in ctx.kernel_name
    states = np.array([np.concatenate([c.qpos, c.r[2:]]) for c in cases])
    mocap = np.array([[c.goal[0], c.goal[1], 0.01, 1, 0, 0, 0] for c in cases])
    ctx.set_states(states, np.zeros(E), mocap)
    ctx.set_task_params_batched(weight=np.array([c.spec.weight for c in cases]),
                                norm_parameter=np.array([c.spec.norm_parameter() for c in cases]) if cc.NPARAM[t] else None,
                                parameters=None, risk=np.array([c.spec.risk for c in cases]))
    times = np.tile(np.arange(P) * ((H - 1) * pm.struct.timestep / (P - 1)), (E, 1))
    values = np.tile(np.linspace(-0.5, 0.5, N)[None, :, None, None], (E, 1, P, 2))      # 64 different splines per environment
    ctx.rollout_splines_batched(H, capi.SPLINE_LINEAR, times, values, num_envs=E, n_per_env=N)
    u = cc.U32 if precision == 32 else cc.U64
    worst = (0.0, None)
    for e, c in enumerate(cases):
        first, other = ctx.fetch_trajectory(e * N), ctx.fetch_trajectory(e * N + 1 + e % (N - 1))
        assert np.array_equal(first.residual[0], c.r) and np.array_equal(other.residual[0], c.r), (c.point, first.residual[0], c.r)
        assert np.array_equal(first.costs[:1].view(np.uint64), other.costs[:1].view(np.uint64)), c.point
        ratio = cc.worst_ratio([first.costs[0]], [cc.exact_cost_value(c.spec, c.r)], [cc.bound_cost_value(c.spec, c.r, u)])
        worst = max(worst, (ratio, f"{c.point} risk {c.spec.risk}"))
    ctx.close()
    print(f"\nnorm_value / lane_cost fp{precision}, norm {t}: worst error / bound {worst[0]:.4f} over {E} environments at {worst[1]}")
    assert worst[0] < 1.0, worst
