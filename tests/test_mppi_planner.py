"""GpuBatchMPPIPlanner / GpuMPPIPlanner (mujoco_mpc_amd/planners.py) on the oracle-backed test backend (batch_mppi_oracle_backend.py: the
MPPI update in numpy, in the device's arithmetic and summation order). Both sides of every comparison run the oracle, so equality is
exact. Particle and Cartpole, E = 3 (2 where two suffice), 64 candidates, H <= 16."""
from fractions import Fraction

import numpy as np
import pytest

import mppi_cases as mc
import task_rows
from batch_mppi_oracle_backend import BatchMppiOracleContext
from batch_oracle_backend import BatchOracleContext
from batch_task_oracle_backend import TaskRows
from mujoco_mpc_amd.planners import GpuBatchMPPIPlanner, GpuBatchSamplingPlanner, GpuMPPIPlanner
from mujoco_mpc_amd.task import load_task
from test_batch_planner import initial_states

E, N, STEPS, SEED = 3, 64, 3, 5
COLD, HOT = 1e-300, 1e300     # every loser's weight underflows to exactly 0 / every weight is exactly 1
HORIZON = {"Cartpole": 16, "Particle": 12}
# moderate temperatures: on the scale of the spread of the 64 returns (Cartpole about 0.5, Particle about 0.01 at these states)
MODERATE = {"Cartpole": [0.02, 0.05, 0.2], "Particle": [0.001, 0.003, 0.01]}


class TaskBatchMppiOracleContext(TaskRows, BatchMppiOracleContext):
    pass


def ready(p, task, n=N):
    p.initialize(task.model, task)
    p.num_trajectory_ = n
    p.allocate()
    p.reset(HORIZON[task.name])
    return p


def fleet(task, temperature, num_envs=E, seed=SEED, backend=BatchMppiOracleContext):
    return ready(GpuBatchMPPIPlanner(num_envs, seed=seed, temperature=temperature, backend_factory=lambda t: backend(t)), task)


def advance(task, states, trajectories):
    """every environment two planning steps along the given trajectory"""
    nq = task.model.nq
    for st, tr in zip(states, trajectories):
        mp = st.mocap.reshape(-1, 7)
        st.set(tr.states[2, :nq], tr.states[2, nq:], mocap_pos=mp[:, :3] if len(mp) else None, mocap_quat=mp[:, 3:] if len(mp) else None,
               time=float(tr.times[2]))


def same_policy(a, b):
    return np.array_equal(a.policy.plan.times(), b.policy.plan.times()) and mc.same_bits(a.policy.plan.values(), b.policy.plan.values())


@pytest.mark.parametrize("name", ["Cartpole", "Particle"])
def test_at_a_vanishing_temperature_mppi_is_predictive_sampling(name, cartpole, particle):
    task = cartpole if name == "Cartpole" else particle
    H = HORIZON[name]
    mppi = fleet(task, COLD)
    ps = ready(GpuBatchSamplingPlanner(E, seed=SEED, backend_factory=lambda t: BatchOracleContext(t)), task)
    assert not hasattr(mppi, "pruning") and hasattr(ps, "pruning")
    states = initial_states(task, name)
    for step in range(STEPS):
        for p in (mppi, ps):
            p.set_states(states)
            p.optimize_policy(H)
        ret = mppi.ctx.returns()[0].reshape(E, N)
        for e in range(E):
            assert (ret[e] == ret[e].min()).sum() == 1, (step, e)       # no tie at the minimum: the one weight of 1 is the winner's
            a, b = mppi.envs[e], ps.envs[e]
            assert a.winner == b.winner and same_policy(a, b), (step, e)
            assert (a.best_return, a.nominal_return, a.improvement) == (b.best_return, b.nominal_return, b.improvement)
            assert a.valid == 1 and a.weight_sum == 1.0 and a.effective_samples == 1.0
            ta, tb = mppi.best_trajectory(e), ps.best_trajectory(e)
            assert np.array_equal(ta.states, tb.states) and np.array_equal(ta.actions, tb.actions) and ta.total_return == tb.total_return
        advance(task, states, [ps.best_trajectory(e) for e in range(E)])
    assert len({p.winner for p in mppi.envs} | {0}) > 1                 # somebody left the nominal


@pytest.mark.parametrize("name", ["Cartpole", "Particle"])
def test_a_fleets_member_is_the_single_planner(name, cartpole, particle):
    task = cartpole if name == "Cartpole" else particle
    H, lam = HORIZON[name], MODERATE[name]
    batch = fleet(task, lam)
    singles = [ready(GpuMPPIPlanner(seed=SEED + e, temperature=lam[e], backend_factory=lambda t: BatchMppiOracleContext(t)), task) for e in range(E)]
    states = initial_states(task, name)
    dt = task.model.get_number("agent_timestep", task.model.timestep)
    for step in range(2):
        batch.set_states(states)
        batch.optimize_policy(H)
        for e, p in enumerate(singles):
            p.set_state(states[e])
            p.optimize_policy(H)
            b = batch.envs[e]
            assert b.winner == p.winner and same_policy(b, p), (step, e)
            for k in ("best_return", "nominal_return", "improvement", "effective_samples", "weight_sum", "valid"):
                assert getattr(b, k) == getattr(p, k), (step, e, k)
            assert 1.0 < p.effective_samples < N - 1 and p.weight_sum > 1.0  # an average: neither the argmin nor the plain mean
            x, y = np.zeros(task.model.nu), np.zeros(task.model.nu)
            batch.action_from_policy(e, x, None, states[e].time + 0.5 * dt)
            p.action_from_policy(y, None, states[e].time + 0.5 * dt)
            assert np.array_equal(x, y)
            tb, ts = batch.best_trajectory(e), p.best_trajectory()
            assert np.array_equal(tb.states, ts.states) and tb.total_return == ts.total_return == p.best_return
        advance(task, states, [p.best_trajectory() for p in singles])
    assert singles[0].temperature == lam[0] and singles[0].num_parameters() == batch.num_parameters()


def test_at_a_huge_temperature_the_policy_is_the_plain_mean_of_the_candidates(particle):
    H = HORIZON["Particle"]
    p = fleet(particle, HOT, num_envs=2)
    p.set_states(initial_states(particle, "Particle")[:2])
    p.optimize_policy(H)
    nodes = p.ctx.nodes.reshape(2, N, -1)
    for e in range(2):
        assert p.envs[e].weight_sum == N and p.envs[e].effective_samples == N
        got = p.envs[e].policy.plan.values().reshape(-1)
        for j in range(nodes.shape[2]):
            col = [Fraction(float(v)) for v in nodes[e, :, j]]
            s, a = sum(col), sum(abs(v) for v in col)
            assert mc.ratio(got[j], s / N, mc.mean_bound(N, a, s, Fraction(N))) <= 1.0, (e, j)
    assert np.abs(p.envs[0].policy.plan.values()).max() > 0


def test_a_temperature_per_member_acts_per_member(particle):
    H = HORIZON["Particle"]
    states = initial_states(particle, "Particle")
    lam = [COLD, 0.003, HOT]
    mixed = fleet(particle, lam)
    assert np.array_equal(mixed.temperature, lam)
    for e in range(E):
        uniform = fleet(particle, lam[e])
        for p in (mixed, uniform) if e == 0 else (uniform,):
            p.set_states(states)
            p.optimize_policy(H)
        assert same_policy(mixed.envs[e], uniform.envs[e]) and mixed.envs[e].weight_sum == uniform.envs[e].weight_sum, e
    assert mixed.envs[0].weight_sum == 1.0 < mixed.envs[1].weight_sum < mixed.envs[2].weight_sum == N
    mixed.temperature = 2.0                                            # settable between plan steps; a scalar is every member's
    assert np.array_equal(mixed.temperature, [2.0] * E)
    for bad in (0.0, -1.0, np.nan, np.inf, [1.0, 2.0]):
        with pytest.raises(ValueError):
            mixed.temperature = bad


def test_a_member_whose_returns_are_all_nan_keeps_its_policy(particle):
    H = HORIZON["Particle"]
    p = fleet(particle, 1.0)
    states = initial_states(particle, "Particle")
    p.set_states(states)
    p.optimize_policy(H)
    before = [(q.policy.plan.times().copy(), q.policy.plan.values().copy()) for q in p.envs]
    p.ctx.nan_envs = (1,)
    p.optimize_policy(H)                                               # the same states: the nominal is resampled at the same times
    q = p.envs[1]
    assert q.valid == 0 and q.weight_sum == 0.0 and q.effective_samples == 0.0 and np.isnan(q.best_return) and q.winner == 0
    assert np.array_equal(q.policy.plan.times(), before[1][0]) and mc.same_bits(q.policy.plan.values(), before[1][1])
    for e in (0, 2):
        assert p.envs[e].valid == 1 and not np.array_equal(p.envs[e].policy.plan.values(), before[e][1])


def test_the_temperature_comes_from_the_model_or_is_an_error():
    task = load_task("Particle")                                       # (a task of this test's own: its model's numerics are edited)
    assert "mppi_temperature" not in task.model.numeric
    for p in (GpuBatchMPPIPlanner(2, backend_factory=lambda t: BatchMppiOracleContext(t)), GpuMPPIPlanner(backend_factory=lambda t: BatchMppiOracleContext(t))):
        with pytest.raises(ValueError, match="mppi_temperature"):
            p.initialize(task.model, task)
    task.model.numeric["mppi_temperature"] = np.array([0.25])
    p = GpuBatchMPPIPlanner(2, backend_factory=lambda t: BatchMppiOracleContext(t))
    p.initialize(task.model, task)
    assert np.array_equal(p.temperature, [0.25, 0.25])
    task.model.numeric["mppi_temperature"] = np.array([4.0])
    p.initialize(task.model, task)                                     # the model's is read again; one that was given stays
    assert np.array_equal(p.temperature, [4.0, 4.0])
    g = GpuMPPIPlanner(temperature=3.0)
    g.initialize(task.model, task)
    assert g.temperature == 3.0


def test_set_tasks_rows_reach_the_members(particle):
    H = HORIZON["Particle"]
    tasks = task_rows.unlike_tasks(particle, E)
    batch = fleet(particle, 0.003, backend=TaskBatchMppiOracleContext)
    batch.set_tasks(tasks)
    st = initial_states(particle, "Particle")[0]
    states = [st] * E                                                  # one state: only the rows tell the members apart
    singles = [ready(GpuMPPIPlanner(seed=SEED + e, temperature=0.003, backend_factory=lambda t: BatchMppiOracleContext(t)), tasks[e]) for e in range(E)]
    batch.set_states(states)
    batch.optimize_policy(H)
    for e, p in enumerate(singles):
        p.set_state(st)
        p.optimize_policy(H)
        b = batch.envs[e]
        assert b.winner == p.winner and same_policy(b, p) and b.nominal_return == p.nominal_return and b.weight_sum == p.weight_sum, e
    assert len({p.nominal_return for p in batch.envs}) == E
