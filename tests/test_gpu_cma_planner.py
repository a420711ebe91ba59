"""-m gpu: GpuBatchCMAESPlanner / GpuCMAESPlanner on the device.
  1. The device planner against the same planner on the oracle backend (candidates and update in numpy), policies, step sizes and
     best returns at 1e-9 (1 + |x|) over two plan steps on Particle and Cartpole (n = 64, H <= 16) -- the tolerance of
     tests/test_gpu_mppi_planner.py for the same comparison. The ranking is a discrete decision: the oracle's mu + 1 best returns of
     the ranked candidates are separated by more than that tolerance (asserted), so both sides rank alike.
  2. A fleet's member is the single planner with seed + e, bit for bit, on the lane kernel (Particle).
  3. The same for two A1s on the quad kernel (n = 64, H = 6), and with set_models on two A1 variants."""
import numpy as np
import pytest

import test_batch_models as cpu
import test_cma_planner as tc
import test_mppi_planner as tm
from batch_cmaes_oracle_backend import BatchCmaOracleContext
from mujoco_mpc_amd.planners import GpuBatchCMAESPlanner, GpuCMAESPlanner
from mujoco_mpc_amd.task import load_task
from selection_cases import same_bits
from test_batch_planner import initial_states
from test_gpu_batch import err
from test_gpu_mppi_planner import assert_same_plan, quad_factory, ready

pytestmark = pytest.mark.gpu
SEED, N, TOL = tm.SEED, tm.N, 1e-9
KEYS = ("best_return", "nominal_return", "improvement", "sigma", "restarted", "valid")


def same_state(a, b, d, ea=0, eb=0):
    sa, sb = a.ctx.cma_get_state_batched(a.num_envs, d), b.ctx.cma_get_state_batched(b.num_envs, d)
    return all(same_bits(np.asarray(sa[k][ea], np.float64), np.asarray(sb[k][eb], np.float64)) for k in tc.STATE_KEYS)


@pytest.mark.parametrize("name", ["Particle", "Cartpole"])
def test_device_planner_against_the_oracle_backend(name):
    task = load_task(name)
    E, H = tm.E, tm.HORIZON[name]
    dev = ready(GpuBatchCMAESPlanner(E, seed=SEED), task, H)
    ref = ready(GpuBatchCMAESPlanner(E, seed=SEED, backend_factory=lambda t: BatchCmaOracleContext(t, threads=16)), task, H)
    states = initial_states(task, name)
    d, mu = dev.num_parameters(), (N - 1) // 2
    worst = 0.0
    for step in range(2):
        for p in (dev, ref):
            p.set_states(states)
            p.optimize_policy(H)
        ret = ref.ctx.returns()[0].reshape(E, N)
        sd, sr = dev.ctx.cma_get_state_batched(E, d), ref.ctx.cma_get_state_batched(E, d)
        for e in range(E):
            ranked = np.sort(ret[e, 1:])[:mu + 1]
            gaps = np.diff(ranked) / (1.0 + np.abs(ranked[1:]))
            assert gaps.min() > TOL, (step, e, gaps.min())               # the mu + 1 best are apart: the same ranking on both sides
            a, b = dev.envs[e], ref.envs[e]
            assert np.array_equal(a.policy.plan.times(), b.policy.plan.times()) and a.winner == b.winner and a.valid == b.valid == 1
            worst = max(worst, err(a.policy.plan.values(), b.policy.plan.values()), err(a.sigma, b.sigma), err(a.best_return, b.best_return),
                        *[err(sd[k][e], sr[k][e]) for k in ("C", "A", "p_sigma", "p_c")])
            assert a.restarted == b.restarted == 0 and a.sigma != dev.envs[e].noise_exploration[0]
        assert np.array_equal(sd["generation"], sr["generation"]) and np.all(sd["generation"] == step + 1)
        tm.advance(task, states, [ref.best_trajectory(e) for e in range(E)])
    print(f"{name}: worst error of policies, step sizes, best returns and the distribution against the oracle backend {worst:.3e}")
    assert worst <= TOL
    dev.ctx.close()


def test_a_fleets_member_is_the_single_planner_on_the_device():
    name = "Particle"
    task = load_task(name)
    E, H = tm.E, tm.HORIZON[name]
    batch = ready(GpuBatchCMAESPlanner(E, seed=SEED, generations=2), task, H)
    singles = [ready(GpuCMAESPlanner(seed=SEED + e, generations=2), task, H) for e in range(E)]
    states = initial_states(task, name)
    d = batch.num_parameters()
    for step in range(2):
        batch.set_states(states)
        batch.optimize_policy(H)
        for e, p in enumerate(singles):
            p.set_state(states[e])
            p.optimize_policy(H)
            assert_same_plan(batch.envs[e], p, (step, e))
            for k in KEYS:
                assert getattr(batch.envs[e], k) == getattr(p, k), (step, e, k)
            assert same_state(batch, p.fleet, d, e, 0), (step, e)
            cpu.tr.assert_same_trajectory(batch.best_trajectory(e), p.best_trajectory(), (step, e))
        tm.advance(task, states, [p.best_trajectory() for p in singles])
    assert np.all(batch.ctx.cma_get_state_batched(E, d)["generation"] == 4)
    for p in [batch] + singles:
        p.ctx.close()


@pytest.mark.parametrize("variants", [False, True], ids=["two-a1s", "two-variants"])
def test_two_a1s_on_the_quad_kernel(variants):
    made = []
    if variants:
        task, models, tasks = cpu.fleet_models()
        factory = None
    else:
        task = load_task("QuadrupedFlat")
        task.transition(0.0)
        tasks, factory = [task, task], quad_factory(made)
    E, H = 2, 6
    batch = ready(GpuBatchCMAESPlanner(E, seed=SEED, sigma0=0.05, backend_factory=factory), task, H)
    if variants:
        batch.set_models(models[:E])
    singles = [ready(GpuCMAESPlanner(seed=SEED + e, sigma0=0.05, backend_factory=factory), tasks[e], H) for e in range(E)]
    if not variants:
        assert "rollout_quad_kernel" in batch.ctx.kernel_name, batch.ctx.kernel_name
    made = made or [batch.ctx] + [p.ctx for p in singles]
    states = [cpu.tr.initial_states(task)[0] for _ in range(E)] if variants else cpu.tr.initial_states(task)[:E]
    d = batch.num_parameters()
    for step in range(2):
        batch.set_states(states)
        batch.optimize_policy(H)
        for e, p in enumerate(singles):
            p.set_state(states[e])
            p.optimize_policy(H)
            assert_same_plan(batch.envs[e], p, (step, e))
            for k in KEYS:
                assert getattr(batch.envs[e], k) == getattr(p, k), (step, e, k)
            assert same_state(batch, p.fleet, d, e, 0), (step, e)
            cpu.tr.assert_same_trajectory(batch.best_trajectory(e), p.best_trajectory(), (step, e))
        tm.advance(task, states, [p.best_trajectory() for p in singles])
    assert batch.envs[0].nominal_return != batch.envs[1].nominal_return and all(p.valid == 1 for p in singles)
    for c in made:
        c.close()
