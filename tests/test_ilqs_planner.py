"""iLQS on the CPU: the policy conversion (mjpc::SplineFit, exported as mjpc_ilqs_fit_spline, and its numpy mirror
planners.fit_spline) against np.linalg.lstsq, and the planner's host logic (planners.GpuILQSPlanner) on the oracle-backed
backend."""
import numpy as np
import pytest

from mujoco_mpc_amd.hostplanner import ilqs_fit_spline
from mujoco_mpc_amd.planners import GpuILQGPlanner, GpuILQSPlanner, State, fit_spline
from mujoco_mpc_amd.spline import TimeSpline
from oracle_backend import OracleContext

T0 = 0.37


def sampling_layout(interp, P, steps, dt):
    """node times as GpuSamplingPlanner::UpdateNominalPolicy lays them out and step times as the rollouts count them, both by
    repeated addition from T0"""
    time_horizon = steps * dt
    shift = max(time_horizon / P, 1e-5) if interp == 0 else (max(time_horizon / (P - 1), 1e-5) if P > 1 else np.inf)
    nodes, t = [], T0
    for _ in range(P):
        nodes.append(t)
        t += shift
    times, t = [], T0
    for _ in range(steps):
        times.append(t)
        t += dt
    return np.array(nodes), np.array(times)


def mapping(interp, node_times, step_times):
    P = len(node_times)
    s = TimeSpline(P, interp)
    for k in range(P):
        s.add_node(node_times[k], np.eye(P)[k])
    return np.array([s.sample(t) for t in step_times])


def close(a, b, tol):
    return np.all(np.abs(np.asarray(a) - np.asarray(b)) <= tol * (1 + np.abs(np.asarray(b))))


@pytest.mark.parametrize("P", [1, 2, 3, 5, 10, 30])
@pytest.mark.parametrize("interp", [0, 1, 2])
def test_fit_matches_lstsq(interp, P):
    rng = np.random.default_rng(10 * P + interp)
    nu = 3
    for steps in sorted({P, 35, 100}):
        node_times, step_times = sampling_layout(interp, P, steps, 0.01)
        M = mapping(interp, node_times, step_times)
        norm = np.linalg.norm(M, axis=0)
        reached = norm > 1e-9 * norm.max()
        actions = rng.uniform(-1, 1, (steps, nu))
        got, status, unreached = ilqs_fit_spline(interp, node_times, step_times, actions)
        assert status == (0 if reached.all() else 1) and unreached == int((~reached).sum())
        want = np.zeros((P, nu))
        for k in np.flatnonzero(~reached):      # the rule: the action at the nearest step time
            want[k] = actions[np.argmin(np.abs(step_times - node_times[k]))]
        want[reached] = np.linalg.lstsq(M[:, reached], actions - M[:, ~reached] @ want[~reached], rcond=None)[0]
        mirror, mstatus, _ = fit_spline(interp, node_times, step_times, actions)
        assert mstatus == status and np.all(np.isfinite(got))
        # the normal equations square M's condition number: the square linear / cubic layouts (P = 30 nodes for 30 steps, the last
        # node barely reached) have cond(M) ~ 1e8, where no bound of this size holds for them or for lstsq
        if np.linalg.cond(M[:, reached]) > 1e4:
            continue
        assert close(got, want, 1e-10), (steps, np.abs(got - want).max())
        assert close(mirror, want, 1e-10)
        # a spline's own in-range samples give back its nodes
        if reached.all():
            nodes = rng.uniform(-1, 1, (P, nu))
            samples = M @ nodes
            back, status, _ = ilqs_fit_spline(interp, node_times, step_times, samples)
            assert status == 0 and close(back, nodes, 1e-10), (steps, np.abs(back - nodes).max())
        # the clamped fit is the clipped unclamped fit
        bounds = np.array([[-0.3, 0.2], [-1.0, 1.0], [0.0, 0.5]])
        clamped, _, _ = ilqs_fit_spline(interp, node_times, step_times, 3 * actions, bounds)
        free, _, _ = ilqs_fit_spline(interp, node_times, step_times, 3 * actions)
        np.testing.assert_array_equal(clamped, np.clip(free, bounds[:, 0], bounds[:, 1]))


def test_fit_on_the_particle_layout():
    """Particle: agent_horizon 1, agent_timestep 0.1 and 11 cubic nodes for 10 actions. Node and step times coincide, so the last
    node reaches no step: it takes the last action, and the other ten reproduce the actions (the reference's Cholesky of the
    singular M^T M gives non-finite parameters here)."""
    from mujoco_mpc_amd.task import load_task
    task = load_task("Particle")
    m = task.model
    H = task.planning_steps()
    P = int(m.get_number("sampling_spline_points", 0))
    dt = m.get_number("agent_timestep", m.timestep)
    assert (H, P, int(m.get_number("sampling_representation", 2))) == (11, 11, 2)
    node_times, step_times = sampling_layout(2, P, H - 1, dt)
    actions = np.random.default_rng(3).uniform(-1, 1, (H - 1, m.nu))
    got, status, unreached = ilqs_fit_spline(2, node_times, step_times, actions, m.actuator_ctrlrange)
    assert status == 1 and unreached == 1
    assert np.all(np.isfinite(got))
    bounds = np.asarray(m.actuator_ctrlrange, float).reshape(-1, 2)
    assert np.all(got >= bounds[:, 0]) and np.all(got <= bounds[:, 1])
    M = mapping(2, node_times, step_times)
    assert np.abs(M @ got - actions).max() < 1e-10
    np.testing.assert_array_equal(got[P - 1], actions[np.argmin(np.abs(step_times - node_times[P - 1]))])
    mirror, mstatus, munreached = fit_spline(2, node_times, step_times, actions, m.actuator_ctrlrange)
    assert (mstatus, munreached) == (1, 1) and close(mirror, got, 1e-12)


def test_fit_refuses_bad_input():
    with pytest.raises(ValueError, match="strictly increasing"):
        ilqs_fit_spline(1, [0.0, 0.0], [0.0, 0.1], np.zeros((2, 1)))
    with pytest.raises(ValueError, match="interpolation"):
        ilqs_fit_spline(3, [0.0, 0.1], [0.0, 0.1], np.zeros((2, 1)))


def particle_planners(iterations, goal_iterations=0):
    from mujoco_mpc_amd.task import load_task
    task = load_task("Particle")
    factory = lambda t: OracleContext(t, differentiable=True)
    ilqs = GpuILQSPlanner(backend_factory=factory)
    ilqs.initialize(task.model, task)
    ilqs.sampling.num_trajectory_ = 1            # only the nominal: sampling never wins
    ilqs.allocate()
    ilqg = GpuILQGPlanner(backend_factory=factory)
    ilqg.initialize(task.model, task)
    ilqg.allocate()
    H = int(max(min(2.5 / 0.1 + 1, 512), 1))    # ilqg_test.cc:75-79
    for p in (ilqs, ilqg):
        p.reset(512)
    st = State(task.model)
    st.set([0.0, 0.0], [0.0, 0.0])
    ilqs.set_state(st)
    ilqg.set_state(st)
    return task, ilqs, ilqg, st, H


def test_mirror_with_one_sample_is_ilqg():
    """with one sampling candidate iLQS is iLQG: iLQG is active after every iteration, its policy is a standalone iLQG
    planner's, and the goal is reached (the ilqg_test.cc criterion)"""
    task, ilqs, ilqg, st, H = particle_planners(25)
    for k in range(25):
        ilqs.optimize_policy(H)
        assert ilqs.active_policy == ilqs.ILQG and ilqs.ilqg_ran and ilqs.ilqg.iteration_completed
        assert ilqs.fit_status == (-1 if k == 0 else 0)   # 11 nodes for 25 actions: every node reached
        if k < 10:
            ilqg.optimize_policy(H)
            a, b = ilqs.ilqg.policy.trajectory, ilqg.policy.trajectory
            assert close(a.actions[:H], b.actions[:H], 1e-9) and close(a.states[:H], b.states[:H], 1e-9)
            assert close(ilqs.ilqg.policy.feedback_gain[:H], ilqg.policy.feedback_gain[:H], 1e-9)
    tr = ilqs.ilqg.candidate0.trajectory
    assert abs(tr.states[H - 1, 0] - st.mocap[0]) < 1e-2 and abs(tr.states[H - 1, 1] - st.mocap[1]) < 1e-2
    assert abs(tr.states[H - 1, 2]) < 1e-1 and abs(tr.states[H - 1, 3]) < 1e-1
    assert np.all(np.abs(tr.actions[:H - 1]) <= 1.0)


def test_action_from_policy_branches():
    """the four branches of ActionFromPolicy (ilqs/planner.cc:228-253), each reached by running the planner"""
    task, ilqs, _, st, H = particle_planners(0)
    nu = task.model.nu
    x = np.array([0.05, -0.02, 0.1, 0.0])

    def action(use_previous, half, previous):
        want = np.zeros(nu)
        getattr(ilqs, half).action_from_policy(want, x, 0.13, previous)
        got = np.zeros(nu)
        ilqs.action_from_policy(got, x, 0.13, use_previous)
        np.testing.assert_array_equal(got, want)

    ilqs.optimize_policy(H)                                       # sampling -> iLQG
    assert (ilqs.previous_active_policy, ilqs.active_policy) == (ilqs.SAMPLING, ilqs.ILQG)
    action(True, "sampling", True)
    action(False, "ilqg", False)
    ilqs.optimize_policy(H)                                       # iLQG -> iLQG
    assert (ilqs.previous_active_policy, ilqs.active_policy) == (ilqs.ILQG, ilqs.ILQG)
    action(True, "ilqg", True)
    action(False, "ilqg", False)
    # iLQG -> sampling: many wide samples around the fitted plan after the goal has moved
    ilqs.sampling.num_trajectory_ = 64
    ilqs.sampling.noise_exploration[0] = 0.5
    st.set([0.0, 0.0], [0.0, 0.0], mocap_pos=[[0.25, -0.25, 0.0]], mocap_quat=[[1.0, 0, 0, 0]])
    ilqs.set_state(st)
    ilqs.optimize_policy(H)
    assert (ilqs.previous_active_policy, ilqs.active_policy) == (ilqs.ILQG, ilqs.SAMPLING) and not ilqs.ilqg_ran
    action(True, "ilqg", False)                                   # iLQG was not updated: its current policy is the previous one
    action(False, "sampling", False)
