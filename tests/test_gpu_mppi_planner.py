"""-m gpu: GpuBatchMPPIPlanner / GpuMPPIPlanner on the device.
  1. At a temperature so small that every loser's weight underflows to 0 the planner IS GpuBatchSamplingPlanner, bit for bit over three
     plan steps (policies, winners, best trajectories): Particle on the lane kernel, QuadrupedFlat (E = 2, 64 candidates, H = 8) on the
     quad kernel. No tie at the minimum (asserted).
  2. The device planner against the same planner on the oracle backend (the update in numpy), policies at 1e-9 (1 + |x|) over two plan
     steps at a moderate temperature -- the tolerance of the fp64 planner parity tests.
  3. A fleet's member is the single planner with seed + e, bit for bit.
  4. With set_models on two A1 variants the plan runs and member e is the single planner created on models[e], bit for bit."""
import numpy as np
import pytest

import mppi_cases as mc
import test_batch_models as cpu
import test_mppi_planner as tm
from batch_mppi_oracle_backend import BatchMppiOracleContext
from mujoco_mpc_amd.planners import GpuBatchMPPIPlanner, GpuBatchSamplingPlanner, GpuMPPIPlanner
from mujoco_mpc_amd.task import load_task
from test_batch_planner import initial_states
from test_gpu_batch import context, err

pytestmark = pytest.mark.gpu
SEED, N = tm.SEED, tm.N


def quad_factory(made):
    def factory(t):
        made.append(context(t.packed_model(), t.packed(), 64, {"MJPCX_QUAD_MIN_N": "0"}))
        return made[-1]
    return factory


def ready(p, task, horizon, exploration=None):
    p.initialize(task.model, task)
    p.num_trajectory_ = N
    if exploration is not None:
        for q in getattr(p, "envs", None) or p.fleet.envs:
            q.noise_exploration = [exploration, 0.0]
    p.allocate()
    p.reset(horizon)
    return p


def assert_same_plan(a, b, where):
    assert a.winner == b.winner, where
    assert np.array_equal(a.policy.plan.times(), b.policy.plan.times()) and mc.same_bits(a.policy.plan.values(), b.policy.plan.values()), where


@pytest.mark.parametrize("name", ["Particle", "QuadrupedFlat"])
def test_at_a_vanishing_temperature_mppi_is_predictive_sampling_on_the_device(name):
    task = load_task(name)
    made = []
    if name == "QuadrupedFlat":
        task.transition(0.0)
        E, H, factory, exploration = 2, 8, quad_factory(made), 0.05
        states = cpu.tr.initial_states(task)[:E]
    else:
        E, H, factory, exploration = 3, tm.HORIZON[name], None, None
        states = initial_states(task, name)
    mppi = ready(GpuBatchMPPIPlanner(E, seed=SEED, temperature=tm.COLD, backend_factory=factory), task, H, exploration)
    ps = ready(GpuBatchSamplingPlanner(E, seed=SEED, backend_factory=factory), task, H, exploration)
    assert ("rollout_quad_kernel" in mppi.ctx.kernel_name) == (name == "QuadrupedFlat"), mppi.ctx.kernel_name
    for step in range(3):
        for p in (mppi, ps):
            p.set_states(states)
            p.optimize_policy(H)
        ret = mppi.ctx.returns()[0].reshape(E, N)
        for e in range(E):
            assert (ret[e] == ret[e].min()).sum() == 1, (step, e)
            a, b = mppi.envs[e], ps.envs[e]
            assert_same_plan(a, b, (name, step, e))
            assert (a.best_return, a.nominal_return, a.improvement) == (b.best_return, b.nominal_return, b.improvement), (step, e)
            assert a.valid == 1 and a.weight_sum == 1.0 and a.effective_samples == 1.0
            cpu.tr.assert_same_trajectory(mppi.best_trajectory(e), ps.best_trajectory(e), (name, step, e))
        tm.advance(task, states, [ps.best_trajectory(e) for e in range(E)])
    for c in made or [mppi.ctx, ps.ctx]:
        c.close()


@pytest.mark.parametrize("name", ["Particle", "Cartpole"])
def test_device_planner_against_the_oracle_backend(name):
    task = load_task(name)
    E, H, lam = tm.E, tm.HORIZON[name], tm.MODERATE[name]
    dev = ready(GpuBatchMPPIPlanner(E, seed=SEED, temperature=lam), task, H)
    ref = ready(GpuBatchMPPIPlanner(E, seed=SEED, temperature=lam, backend_factory=lambda t: BatchMppiOracleContext(t, threads=16)), task, H)
    states = initial_states(task, name)
    worst = 0.0
    for step in range(2):
        for p in (dev, ref):
            p.set_states(states)
            p.optimize_policy(H)
        for e in range(E):
            a, b = dev.envs[e], ref.envs[e]
            assert np.array_equal(a.policy.plan.times(), b.policy.plan.times())
            worst = max(worst, err(a.policy.plan.values(), b.policy.plan.values()), err(a.effective_samples, b.effective_samples),
                        err(a.best_return, b.best_return))
            assert 1.0 < b.effective_samples < N - 1, (step, e, b.effective_samples)     # an average, not the argmin or the plain mean
        tm.advance(task, states, [ref.best_trajectory(e) for e in range(E)])
    print(f"{name}: worst error of policies, effective samples and best returns against the oracle backend {worst:.3e}")
    assert worst <= 1e-9
    dev.ctx.close()


def test_a_fleets_member_is_the_single_planner_on_the_device():
    name = "Particle"
    task = load_task(name)
    E, H, lam = tm.E, tm.HORIZON[name], tm.MODERATE[name]
    batch = ready(GpuBatchMPPIPlanner(E, seed=SEED, temperature=lam), task, H)
    singles = [ready(GpuMPPIPlanner(seed=SEED + e, temperature=lam[e]), task, H) for e in range(E)]
    states = initial_states(task, name)
    for step in range(2):
        batch.set_states(states)
        batch.optimize_policy(H)
        for e, p in enumerate(singles):
            p.set_state(states[e])
            p.optimize_policy(H)
            assert_same_plan(batch.envs[e], p, (step, e))
            for k in ("best_return", "nominal_return", "improvement", "effective_samples", "weight_sum", "valid"):
                assert getattr(batch.envs[e], k) == getattr(p, k), (step, e, k)
            cpu.tr.assert_same_trajectory(batch.best_trajectory(e), p.best_trajectory(), (step, e))
        tm.advance(task, states, [p.best_trajectory() for p in singles])
    for p in [batch] + singles:
        p.ctx.close()


def test_a_fleet_of_two_a1_variants_is_one_planner_per_model():
    task, models, tasks = cpu.fleet_models()
    E, H, lam = 2, 8, [0.002, 0.01]
    batch = ready(GpuBatchMPPIPlanner(E, seed=SEED, temperature=lam), task, H, 0.05)
    batch.set_models(models[:E])
    singles = [ready(GpuMPPIPlanner(seed=SEED + e, temperature=lam[e]), tasks[e], H, 0.05) for e in range(E)]
    made = [batch.ctx] + [p.ctx for p in singles]
    states = [cpu.tr.initial_states(task)[0] for _ in range(E)]           # ONE state: the models (and the seeds) tell the robots apart
    for step in range(2):
        batch.set_states(states)
        batch.optimize_policy(H)
        for e, p in enumerate(singles):
            p.set_state(states[e])
            p.optimize_policy(H)
            assert_same_plan(batch.envs[e], p, (step, e))
            assert batch.envs[e].effective_samples == p.effective_samples and batch.envs[e].valid == p.valid == 1, (step, e)
            cpu.tr.assert_same_trajectory(batch.best_trajectory(e), p.best_trajectory(), (step, e))
        tm.advance(task, states, [p.best_trajectory() for p in singles])
    print(f"effective samples of the two robots: {[p.effective_samples for p in singles]}")
    assert batch.envs[0].nominal_return != batch.envs[1].nominal_return
    for c in made:
        c.close()
