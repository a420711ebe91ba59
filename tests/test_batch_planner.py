"""GpuBatchSamplingPlanner (mujoco_mpc_amd/planners.py) on the oracle-backed test backend: Predictive Sampling for E environments on
one context is, environment by environment, the GpuSamplingPlanner with seed s + e. Both sides run the oracle, so equality is exact."""
import numpy as np
import pytest

from batch_oracle_backend import BatchOracleContext
from mujoco_mpc_amd.planners import GpuBatchSamplingPlanner, GpuSamplingPlanner, State
from oracle_backend import OracleContext

E, N_PER_ENV, STEPS, SEED = 3, 64, 3, 5


def batch_planner(task, n, seed=SEED, num_envs=E):
    p = GpuBatchSamplingPlanner(num_envs, seed=seed, backend_factory=lambda t: BatchOracleContext(t))
    p.initialize(task.model, task)
    p.num_trajectory_ = n
    p.allocate()
    return p


def single_planner(task, n, seed):
    p = GpuSamplingPlanner(seed=seed, backend_factory=lambda t: OracleContext(t))
    p.initialize(task.model, task)
    p.num_trajectory_ = n
    p.allocate()
    return p


def initial_states(task, name):
    """three different states; a different mocap goal per Particle environment"""
    m = task.model
    rng = np.random.default_rng(17)
    out = []
    for e in range(E):
        st = State(m)
        q = rng.uniform(-0.5, 0.5, m.nq) * (1.0 if name == "Cartpole" else 0.2)
        v = rng.normal(0, 0.3, m.nv)
        if m.nmocap:
            st.set(q, v, mocap_pos=[[0.1 * (e + 1), -0.05 * e, 0.01]], mocap_quat=[[1, 0, 0, 0]], time=0.1 * e)
        else:
            st.set(q, v, time=0.1 * e)
        out.append(st)
    return out


@pytest.mark.parametrize("name", ["Cartpole", "Particle"])
def test_batch_planner_is_one_sampling_planner_per_environment(name, cartpole, particle):
    task = cartpole if name == "Cartpole" else particle
    H = 30 if name == "Cartpole" else task.planning_steps()
    batch = batch_planner(task, N_PER_ENV)
    singles = [single_planner(task, N_PER_ENV, SEED + e) for e in range(E)]
    batch.reset(H)
    for p in singles:
        p.reset(H)
    states = initial_states(task, name)
    dt = task.model.get_number("agent_timestep", task.model.timestep)
    for step in range(STEPS):
        batch.set_states(states)
        batch.optimize_policy(H)
        for e, p in enumerate(singles):
            p.set_state(states[e])
            p.optimize_policy(H)
            assert batch.winners[e] == p.winner, (step, e)
            assert np.array_equal(batch.envs[e].policy.plan.times(), p.policy.plan.times()), (step, e)
            assert np.array_equal(batch.envs[e].policy.plan.values(), p.policy.plan.values()), (step, e)
            assert batch.envs[e].best_return == p.best_return and batch.envs[e].nominal_return == p.nominal_return
            a, b = np.zeros(task.model.nu), np.zeros(task.model.nu)
            batch.action_from_policy(e, a, None, states[e].time + 0.5 * dt)
            p.action_from_policy(b, None, states[e].time + 0.5 * dt)
            assert np.array_equal(a, b)
            tb, ts = batch.best_trajectory(e), p.best_trajectory()
            assert np.array_equal(tb.states, ts.states) and tb.total_return == ts.total_return
        # advance every environment along its own best trajectory (two planning steps ahead)
        nq = task.model.nq
        for e in range(E):
            tr = singles[e].best_trajectory()
            mp = states[e].mocap.reshape(-1, 7)
            states[e].set(tr.states[2, :nq], tr.states[2, nq:], mocap_pos=mp[:, :3] if len(mp) else None,
                          mocap_quat=mp[:, 3:] if len(mp) else None, time=float(tr.times[2]))
    # the winners differ between environments somewhere: the three environments were not the same problem
    assert len({tuple(np.round(p.policy.plan.values().ravel(), 12)) for p in singles}) == E


def test_nominal_trajectories_of_all_environments(cartpole):
    H = 20
    batch = batch_planner(cartpole, N_PER_ENV)
    singles = [single_planner(cartpole, N_PER_ENV, SEED + e) for e in range(E)]
    batch.reset(H)
    states = initial_states(cartpole, "Cartpole")
    batch.set_states(states)
    batch.optimize_policy(H)
    noms = batch.nominal_trajectory(H)
    for e, p in enumerate(singles):
        p.reset(H)
        p.set_state(states[e])
        p.optimize_policy(H)
        ref = p.nominal_trajectory(H)
        assert np.array_equal(noms[e].states, ref.states) and noms[e].total_return == ref.total_return


def test_candidates_per_environment_must_be_a_multiple_of_64(cartpole):
    batch = batch_planner(cartpole, 10)
    batch.reset(20)
    batch.set_states(initial_states(cartpole, "Cartpole"))
    with pytest.raises(ValueError, match="multiple of 64"):
        batch.optimize_policy(20)


def test_the_number_of_states_must_match_the_environments(cartpole):
    batch = batch_planner(cartpole, N_PER_ENV)
    with pytest.raises(ValueError, match="3 environments"):
        batch.set_states(initial_states(cartpole, "Cartpole")[:2])
