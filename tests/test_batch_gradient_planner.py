"""GpuBatchGradientPlanner (mujoco_mpc_amd/planners.py) on the oracle-backed test backend: the Gradient planner for E environments on
one context is, environment by environment, a GpuGradientPlanner. Both sides run the oracle and gradient_reference.py, so equality
is exact -- over four consecutive plan steps, with every environment advancing along its own best trajectory."""
import numpy as np
import pytest

from batch_gradient_oracle_backend import BatchGradientOracleContext
from gradient_reference import OracleGradientContext
from mujoco_mpc_amd.planners import GpuBatchGradientPlanner, GpuGradientPlanner, State
from mujoco_mpc_amd.task import load_task

E, N, STEPS = 3, 64, 4


def configure(p, task, n, H, representation, skip):
    p.initialize(task.model, task)
    p.num_trajectory = n
    p.allocate()
    p.reset(H)
    p.derivative_skip_ = skip
    for member in (p.envs if hasattr(p, "envs") else [p]):
        for q in (member.policy, member.previous_policy, member.candidate0):
            q.representation = representation
    return p


def batch_planner(task, H, representation=1, skip=0, n=N, num_envs=E):
    return configure(GpuBatchGradientPlanner(num_envs, backend_factory=lambda t: BatchGradientOracleContext(t, threads=8, differentiable=True)),
                     task, n, H, representation, skip)


def single_planner(task, H, representation=1, skip=0, n=N):
    return configure(GpuGradientPlanner(backend_factory=lambda t: OracleGradientContext(t, threads=8, differentiable=True)), task, n, H,
                     representation, skip)


def fleet(name):
    """the task, a horizon, and three environments with different states, clocks and mocap poses"""
    task = load_task(name)
    m = task.model
    rng = np.random.default_rng(17)
    states = []
    for e in range(E):
        st = State(m)
        if name == "QuadrupedFlat":
            q = np.asarray(m.keyframes["home"]["qpos"], float).copy()
            q[0:2] += 0.05 * e
            q[7:] += rng.normal(0, 0.05, 12)
            v = rng.normal(0, 0.1, 18)
            st.set(q, v, mocap_pos=[[0.3 + 0.2 * e, -0.1 * e, 0.26], [-2.5, 0, 0]], mocap_quat=[[1, 0, 0, 0], [1, 0, 0, 0]], time=0.04 * e)
        elif m.nmocap:
            st.set(rng.uniform(-0.1, 0.1, m.nq), rng.normal(0, 0.3, m.nv), mocap_pos=[[0.1 * (e + 1), -0.05 * e, 0.01]],
                   mocap_quat=[[1, 0, 0, 0]], time=0.1 * e)
        else:
            st.set(rng.uniform(-0.5, 0.5, m.nq), rng.normal(0, 0.3, m.nv), time=0.1 * e)
        states.append(st)
    if name == "QuadrupedFlat":
        task.transition(0.0)
    H = {"Cartpole": 30, "QuadrupedFlat": 12}.get(name, task.planning_steps())
    return task, H, states


@pytest.mark.parametrize("skip", [0, 3])
@pytest.mark.parametrize("representation", [0, 1, 2])
@pytest.mark.parametrize("name", ["Cartpole", "Particle", "QuadrupedFlat"])
def test_batch_planner_is_one_gradient_planner_per_environment(name, representation, skip):
    task, H, states = fleet(name)
    batch = batch_planner(task, H, representation, skip)
    singles = [single_planner(task, H, representation, skip) for _ in range(E)]
    assert batch.num_trajectory == N and batch.derivative_skip_ == skip
    nq = task.model.nq
    improved = 0
    for step in range(STEPS):
        batch.set_states(states)
        batch.optimize_policy(H)
        for e, p in enumerate(singles):
            b = batch.envs[e]
            p.set_state(states[e])
            p.optimize_policy(H)
            P = p.policy.num_spline_points
            assert b.winner == p.winner and batch.winner[e] == p.winner, (step, e)
            assert b.action_step == p.action_step, (step, e)
            assert np.array_equal(b.dV, p.dV), (step, e)
            assert np.array_equal(b.policy.parameters[:P], p.policy.parameters[:P]), (step, e)
            assert np.array_equal(b.policy.times[:P], p.policy.times[:P]), (step, e)
            assert np.array_equal(b.candidate0.parameter_update[:P], p.candidate0.parameter_update[:P]), (step, e)
            assert b.improvement == p.improvement and b.expected == p.expected and b.surprise == p.surprise, (step, e)
            tb, ts = batch.best_trajectory(e), p.best_trajectory()
            assert tb.total_return == ts.total_return, (step, e)
            assert np.array_equal(tb.states, ts.states) and np.array_equal(tb.actions, ts.actions), (step, e)
            x, y = np.zeros(task.model.nu), np.zeros(task.model.nu)
            batch.action_from_policy(e, x, None, states[e].time + 0.004)
            p.action_from_policy(y, None, states[e].time + 0.004)
            assert np.array_equal(x, y)
            improved += p.improvement > 0
        # every environment advances along its own best trajectory (two planning steps ahead)
        for e in range(E):
            tr = singles[e].best_trajectory()
            mp = states[e].mocap.reshape(-1, 7)
            states[e].set(tr.states[2, :nq], tr.states[2, nq:], mocap_pos=mp[:, :3] if len(mp) else None,
                          mocap_quat=mp[:, 3:] if len(mp) else None, time=float(tr.times[2]))
    assert improved > 0
    # the three environments were not the same problem
    P = batch.envs[0].policy.num_spline_points
    assert len({tuple(np.round(p.policy.parameters[:P].ravel(), 12)) for p in batch.envs}) == E


def test_nominal_trajectories_of_all_environments():
    task, H, states = fleet("Particle")
    batch = batch_planner(task, H)
    batch.set_states(states)
    batch.optimize_policy(H)
    noms = batch.nominal_trajectory(H)
    for e in range(E):
        p = single_planner(task, H)
        p.set_state(states[e])
        p.optimize_policy(H)
        p.nominal_trajectory(H)   # (candidate0: the policy the plan step resampled and updated, on both sides)
        assert np.array_equal(noms[e].actions, p.trajectory0.actions) and noms[e].total_return == p.trajectory0.total_return
        assert batch.best_trajectory(e) is noms[e]


def test_the_settings_are_shared_by_all_environments(cartpole):
    batch = batch_planner(cartpole, 20, skip=2)
    batch.num_trajectory = 128
    for p in batch.envs:
        assert (p.num_trajectory, p.derivative_skip_) == (128, 2) and p.settings is batch.settings
    assert batch.num_parameters() == batch.envs[0].num_parameters()


def test_candidates_per_environment_must_be_a_multiple_of_64(cartpole):
    batch = batch_planner(cartpole, 20, n=32)
    batch.set_states(fleet("Cartpole")[2])
    with pytest.raises(ValueError, match="multiple of 64"):
        batch.optimize_policy(20)


def test_the_number_of_states_must_match_the_environments(cartpole):
    batch = batch_planner(cartpole, 20)
    with pytest.raises(ValueError, match="3 environments"):
        batch.set_states(fleet("Cartpole")[2][:2])
    with pytest.raises(ValueError, match="at least one"):
        GpuBatchGradientPlanner(0)
