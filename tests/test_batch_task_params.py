"""Per-environment task weights and parameters without a device: mjpcx_set_task_params_batched is declared, exported and bound, and each
of the four fleet planners with set_tasks of three unlike tasks is, member by member, a single planner created on that member's task.
Both sides run the CPU oracle (tests/batch_task_oracle_backend.py: the batched oracle backends with one packed task per environment),
so equality is exact. Every fleet starts its three environments from the SAME state with DIFFERENT rows -- weights, norm parameters,
residual parameters, risk 0 / positive / negative, and for the A1 also gait, speed and mode through the frozen residual state -- and each
test first asserts that the same spline from that state costs every environment something else: a staging that ignored the rows would
not get that far. Shapes: 64 candidates per environment (iLQG: 10 rollouts), T = 12, two plan steps."""
import os
import re

import numpy as np
import pytest

import task_rows
from batch_task_oracle_backend import (TaskBatchCeOracleContext, TaskBatchGradientOracleContext, TaskBatchILQGOracleContext,
                                       TaskBatchILQGStepOracleContext, TaskBatchOracleContext)
from gradient_reference import OracleGradientContext
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import (GpuBatchCrossEntropyPlanner, GpuBatchGradientPlanner, GpuBatchILQGPlanner, GpuBatchSamplingPlanner,
                                     GpuCrossEntropyPlanner, GpuGradientPlanner, GpuILQGPlanner, GpuSamplingPlanner, State)
from mujoco_mpc_amd.task import load_task
from oracle_backend import OracleContext
from test_batch_ilqg_planner import assert_same_planner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, T, STEPS, SEED = 3, 12, 2, 5
MODELS = ["Cartpole", "Particle", "QuadrupedFlat"]


def test_the_symbol_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mjpcx.h")).read(), flags=re.S)
    assert re.search(r"\bint mjpcx_set_task_params_batched\s*\(", src)
    assert "mjpcx_set_task_params_batched" in capi.EXPORTS
    assert hasattr(capi.lib(), "mjpcx_set_task_params_batched") and callable(getattr(capi.Context, "set_task_params_batched"))
    for cls in (GpuBatchSamplingPlanner, GpuBatchCrossEntropyPlanner, GpuBatchGradientPlanner, GpuBatchILQGPlanner):
        assert callable(getattr(cls, "set_tasks"))


def fleet(name):
    """the task, E States that are ONE state, and E unlike tasks"""
    task = load_task(name)
    m = task.model
    rng = np.random.default_rng(17)
    if name == "QuadrupedFlat":
        q = np.asarray(m.keyframes["home"]["qpos"], float).copy()
        q[7:] += rng.normal(0, 0.05, 12)
        args = dict(qpos=q, qvel=rng.normal(0, 0.1, 18), mocap_pos=[[0.5, -0.1, 0.26], [-2.5, 0, 0]], mocap_quat=[[1, 0, 0, 0], [1, 0, 0, 0]], time=0.04)
        task.transition(0.0)
    elif m.nmocap:
        args = dict(qpos=rng.uniform(-0.1, 0.1, m.nq), qvel=rng.normal(0, 0.3, m.nv), mocap_pos=[[0.2, -0.05, 0.01]], mocap_quat=[[1, 0, 0, 0]], time=0.1)
    else:
        args = dict(qpos=rng.uniform(-0.5, 0.5, m.nq), qvel=rng.normal(0, 0.3, m.nv), time=0.1)
    states = []
    for e in range(E):
        st = State(m)
        st.set(**args)
        states.append(st)
    tasks = task_rows.unlike_tasks(task, E)
    if name == "QuadrupedFlat":   # different gaits and modes: the frozen residual state differs too
        assert len({tuple(t.residual_int) for t in tasks}) > 1 and len({t.current_mode for t in tasks}) > 1
    return task, states, tasks


def assert_rows_decide_the_cost(batch, states, horizon):
    """the zero spline from the one state, under every environment's rows: E different returns"""
    batch.set_states(states)
    batch._push_states()
    nu = batch.model.nu
    batch.ctx.rollout_splines_batched(horizon, capi.SPLINE_ZERO, np.array([[s.time] for s in states]), np.zeros((E, 64, 1, nu)), num_envs=E, n_per_env=64)
    ret, fail = batch.ctx.returns()
    assert not fail.any()
    firsts = [float(ret[64 * e]) for e in range(E)]
    assert len(set(firsts)) == E, firsts
    push = batch.ctx.pushes[-1]
    want = task_rows.rows_of(batch._tasks)
    for k in ("weight", "norm_parameter", "parameters"):
        assert np.array_equal(push[k].reshape(want[k].shape), want[k]), k
    assert np.array_equal(push["risk"].ravel(), want["risk"]) and set(np.sign(want["risk"])) == {0.0, 1.0, -1.0}


def step_along(task, states, singles):
    """every environment advances along its own best trajectory (two planning steps ahead): from here on the states differ as well"""
    nq = task.model.nq
    for e in range(E):
        tr = singles[e].best_trajectory()
        mp = states[e].mocap.reshape(-1, 7)
        states[e].set(tr.states[2, :nq], tr.states[2, nq:], mocap_pos=mp[:, :3] if len(mp) else None, mocap_quat=mp[:, 3:] if len(mp) else None,
                      time=float(tr.times[2]))


def assert_same_trajectory(tb, ts, where):
    assert tb.total_return == ts.total_return and tb.failure == ts.failure, where
    for k in ("states", "actions", "times", "residual", "costs", "trace"):
        assert np.array_equal(getattr(tb, k), getattr(ts, k)), (where, k)


# ---------------------------------------------------------------------------------------------- Predictive Sampling, Cross-Entropy
def sampling(task, tasks=None, seed=SEED):
    p = (GpuBatchSamplingPlanner(E, seed=seed, backend_factory=lambda t: TaskBatchOracleContext(t, threads=8)) if tasks is not None else
         GpuSamplingPlanner(seed=seed, backend_factory=lambda t: OracleContext(t, threads=8)))
    p.initialize(task.model, task)
    p.num_trajectory_ = 64
    if task.name == "QuadrupedFlat":
        for q in (p.envs if tasks is not None else [p]):
            q.noise_exploration = [0.05, 0.0]
    p.allocate()
    if tasks is not None:
        p.set_tasks(tasks)
    p.reset(T)
    return p


def cross_entropy(task, tasks=None, seed=SEED):
    p = (GpuBatchCrossEntropyPlanner(E, seed=seed, backend_factory=lambda t: TaskBatchCeOracleContext(t, threads=8)) if tasks is not None else
         GpuCrossEntropyPlanner(seed=seed, backend_factory=lambda t: OracleContext(t, threads=8)))
    p.initialize(task.model, task)
    p.num_trajectory_ = 63
    p.n_elite_ = 6
    p.explore_fraction_ = 0.1
    if task.name == "QuadrupedFlat":
        p.std_initial_ = 0.05
    p.allocate()
    if tasks is not None:
        p.set_tasks(tasks)
    p.reset(T)
    return p


@pytest.mark.parametrize("name", MODELS)
def test_sampling_fleet_with_tasks_is_one_planner_per_task(name):
    task, states, tasks = fleet(name)
    batch = sampling(task, tasks)
    singles = [sampling(tasks[e], seed=SEED + e) for e in range(E)]
    assert_rows_decide_the_cost(batch, states, T)
    for step in range(STEPS):
        batch.set_states(states)
        batch.optimize_policy(T)
        for e, p in enumerate(singles):
            b = batch.envs[e]
            p.set_state(states[e])
            p.optimize_policy(T)
            assert batch.winners[e] == p.winner, (step, e)
            assert (b.best_return, b.nominal_return, b.improvement) == (p.best_return, p.nominal_return, p.improvement), (step, e)
            assert np.array_equal(b.policy.plan.times(), p.policy.plan.times()) and np.array_equal(b.policy.plan.values(), p.policy.plan.values()), (step, e)
            assert_same_trajectory(batch.best_trajectory(e), p.best_trajectory(), (step, e))
        if step == 0:   # the nominal spline is the same zero policy from the same state: only the rows tell the environments apart
            assert len({p.nominal_return for p in batch.envs}) == E
        step_along(task, states, singles)
    batch.set_states(states)
    noms = batch.nominal_trajectory(T)     # the nominal launch reads the rows as well
    for e, p in enumerate(singles):
        p.set_state(states[e])
        assert_same_trajectory(noms[e], p.nominal_trajectory(T), e)


@pytest.mark.parametrize("name", MODELS)
def test_cross_entropy_fleet_with_tasks_is_one_planner_per_task(name):
    task, states, tasks = fleet(name)
    batch = cross_entropy(task, tasks)
    singles = [cross_entropy(tasks[e], seed=SEED + e) for e in range(E)]
    assert_rows_decide_the_cost(batch, states, T)
    for step in range(STEPS):
        batch.set_states(states)
        batch.optimize_policy(T)
        for e, p in enumerate(singles):
            b = batch.envs[e]
            p.set_state(states[e])
            p.optimize_policy(T)
            assert b.trajectory_order == p.trajectory_order and b.improvement == p.improvement, (step, e)
            assert np.array_equal(b.policy.plan.times(), p.policy.plan.times()) and np.array_equal(b.policy.plan.values(), p.policy.plan.values()), (step, e)
            assert np.array_equal(b.variance, p.variance), (step, e)
            assert_same_trajectory(batch.best_trajectory(e), p.best_trajectory(), (step, e))
        step_along(task, states, singles)


# ---------------------------------------------------------------------------------------------- Gradient
def gradient(task, tasks=None):
    p = (GpuBatchGradientPlanner(E, backend_factory=lambda t: TaskBatchGradientOracleContext(t, threads=8, differentiable=True)) if tasks is not None else
         GpuGradientPlanner(backend_factory=lambda t: OracleGradientContext(t, threads=8, differentiable=True)))
    p.initialize(task.model, task)
    p.num_trajectory = 64
    p.allocate()
    if tasks is not None:
        p.set_tasks(tasks)
    p.reset(T)
    return p


@pytest.mark.parametrize("name", MODELS)
def test_gradient_fleet_with_tasks_is_one_planner_per_task(name):
    task, states, tasks = fleet(name)
    batch = gradient(task, tasks)
    singles = [gradient(tasks[e]) for e in range(E)]
    assert_rows_decide_the_cost(batch, states, T)
    for step in range(STEPS):
        batch.set_states(states)
        batch.optimize_policy(T)
        for e, p in enumerate(singles):
            b = batch.envs[e]
            p.set_state(states[e])
            p.optimize_policy(T)
            P = p.policy.num_spline_points
            assert b.winner == p.winner and b.action_step == p.action_step and np.array_equal(b.dV, p.dV), (step, e)
            assert (b.improvement, b.expected, b.surprise) == (p.improvement, p.expected, p.surprise), (step, e)
            assert np.array_equal(b.policy.parameters[:P], p.policy.parameters[:P]) and np.array_equal(b.policy.times[:P], p.policy.times[:P]), (step, e)
            assert np.array_equal(b.candidate0.parameter_update[:P], p.candidate0.parameter_update[:P]), (step, e)
            assert_same_trajectory(batch.best_trajectory(e), p.best_trajectory(), (step, e))
        if step == 0:   # same state, same zero policy: the gradients differ through the rows alone
            assert len({tuple(b.candidate0.parameter_update[:P].ravel()) for b in batch.envs}) == E
        step_along(task, states, singles)


# ---------------------------------------------------------------------------------------------- iLQG
def ilqg(task, tasks=None, backend=TaskBatchILQGOracleContext, **kw):
    p = (GpuBatchILQGPlanner(E, backend_factory=lambda t: backend(t, threads=8, differentiable=True, **kw)) if tasks is not None else
         GpuILQGPlanner(backend_factory=lambda t: OracleContext(t, threads=8, differentiable=True)))
    p.initialize(task.model, task)
    p.num_rollouts_gui_ = 10
    p.allocate()
    if tasks is not None:
        p.set_tasks(tasks)
    p.reset(T)
    return p


@pytest.mark.parametrize("backend", [TaskBatchILQGOracleContext, TaskBatchILQGStepOracleContext], ids=["sequential", "device_chain"])
@pytest.mark.parametrize("name", MODELS)
def test_ilqg_fleet_with_tasks_is_one_planner_per_task(name, backend):
    task, states, tasks = fleet(name)
    batch = ilqg(task, tasks, backend)
    singles = [ilqg(tasks[e]) for e in range(E)]
    assert_rows_decide_the_cost(batch, states, T)
    for step in range(STEPS):
        batch.set_states(states)
        batch.optimize_policy(T)
        assert batch.used_device_chain == (backend is TaskBatchILQGStepOracleContext)
        for e, p in enumerate(singles):
            p.set_state(states[e])
            p.optimize_policy(T)
            assert_same_planner(batch.envs[e], p, T, (step, e))     # winners, returns, policies, trajectories, regularisation, gains
            assert_same_trajectory(batch.best_trajectory(e), p.best_trajectory(), (step, e))
        if step == 0:
            assert len({p.policy.trajectory.total_return for p in batch.envs}) == E
        step_along(task, states, singles)


def test_ilqg_rows_survive_a_members_sequential_fallback():
    """device chain; environment 1's nominal rollouts are all reported failed, so that member runs the plain sequential chain -- its plain
    set_task_params and set_residual_state on the shared context -- between the two batched launches of the same plan step. The
    environments planned after it (the line search of the same step, everything of the next) still plan with their own rows: members
    0 and 2 equal single planners on their tasks exactly, and member 1 equals the member of a fleet whose middle is sequential
    throughout."""
    task, states, tasks = fleet("QuadrupedFlat")
    chain = ilqg(task, tasks, TaskBatchILQGStepOracleContext, fail_nominal=(1,))

    class FailingPlain(TaskBatchILQGOracleContext):
        def rollout_feedback_batched(self, horizon, mode, *args, **kw):
            super().rollout_feedback_batched(horizon, mode, *args, **kw)
            if mode == 1:
                self.out["failure"][self.n_per_env:2 * self.n_per_env] = 1

    plain = ilqg(task, tasks, FailingPlain)
    singles = [ilqg(tasks[e]) for e in range(E)]
    for step in range(STEPS):
        for p in (chain, plain):
            p.set_states(states)
            p.optimize_policy(T)
        assert chain.used_device_chain and not plain.used_device_chain
        cand, status = chain.ctx.step_calls[-1]
        assert cand[1] == -1 and list(status) == [1, -1, 1]
        assert chain.envs[1].timers["backward_pass"] > 0            # member 1 did run the sequential chain
        assert_same_planner(chain.envs[1], plain.envs[1], T, (step, 1))
        for e in (0, 2):
            singles[e].set_state(states[e])
            singles[e].optimize_policy(T)
            assert_same_planner(chain.envs[e], singles[e], T, (step, e))
        # the fallback's plain calls took the per-environment residual state with them (as the library does) and the planner pushed it back
        assert chain.ctx.rows["residual_int"] is not None and len({tuple(r) for r in chain.ctx.rows["residual_int"]}) > 1
        nq = task.model.nq
        for e in range(E):
            tr = plain.envs[e].best_trajectory()
            mp = states[e].mocap.reshape(-1, 7)
            states[e].set(tr.states[2, :nq], tr.states[2, nq:], mocap_pos=mp[:, :3], mocap_quat=mp[:, 3:], time=float(tr.times[2]))
    assert len(chain.ctx.step_calls) == STEPS


# ---------------------------------------------------------------------------------------------- set_tasks itself
def test_set_tasks_checks_and_reverts(cartpole, particle):
    tasks = task_rows.unlike_tasks(cartpole, E)
    p = GpuBatchSamplingPlanner(E, seed=SEED, backend_factory=lambda t: TaskBatchOracleContext(t))
    with pytest.raises(ValueError, match="before initialize"):
        p.set_tasks(tasks)
    p.initialize(cartpole.model, cartpole)
    p.num_trajectory_ = 64
    p.allocate()
    with pytest.raises(ValueError, match="2 tasks for 3 environments"):
        p.set_tasks(tasks[:2])
    with pytest.raises(ValueError, match="environment 1 differs"):
        p.set_tasks([tasks[0], particle, tasks[2]])
    p.reset(T)
    st = State(cartpole.model)
    st.set([0.3, 2.5], [-0.2, 0.4], time=0.1)
    p.set_states([st] * E)
    p.optimize_policy(T)
    assert p.ctx.pushes == []                                       # without set_tasks: as before, nothing per environment
    p.set_tasks(tasks)
    p.optimize_policy(T)
    assert len(p.ctx.pushes) == 1 and all(b.task is t for b, t in zip(p.envs, tasks))
    p.set_tasks(None)
    p.optimize_policy(T)
    assert all(v is None for v in p.ctx.pushes[-1].values()) and all(b.task is cartpole for b in p.envs)   # everything shared again
