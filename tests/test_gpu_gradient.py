"""-m gpu: the Gradient planner on the device.
   mjpcx_gradient_pass  <-> tests/gradient_reference.py (gradient.cc + spline_mapping.cc restated)      1e-12 (1 + |x|)
   line-search rollouts <-> clamp(interp(theta + s_i * gradient)) of the Python policy                  1e-12
   mjpc::GpuGradientPlanner (C++, GPU) <-> planners.GpuGradientPlanner on the oracle backend           1e-7 relative
The last is looser: the device's and the oracle's finite-difference derivatives differ by about 1e-9 absolute
(tests/test_gpu_ilqg.py)."""
import numpy as np
import pytest

from gradient_reference import OracleGradientContext, gradient_pass
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import GpuGradientPlanner, GradientPolicy, State, clamp, log_scale
from oracle import pyoracle

pytestmark = pytest.mark.gpu

QUAD_MOCAP_POS = np.array([[0.3, 0, 0.26], [-2.5, 0, 0]])
QUAD_MOCAP_QUAT = np.array([[1.0, 0, 0, 0], [1.0, 0, 0, 0]])


def task_and_state(name):
    from mujoco_mpc_amd.task import load_task
    task = load_task(name)
    if name == "QuadrupedFlat":
        task.transition(0.0)
        qpos, qvel = task.model.keyframes["home"]["qpos"], np.zeros(18)
        mocap = np.concatenate([np.concatenate([p, q]) for p, q in zip(QUAD_MOCAP_POS, QUAD_MOCAP_QUAT)])
    elif name == "Cartpole":
        qpos, qvel, mocap = np.array([0.3, 2.5]), np.array([-0.2, 0.4]), None
    else:
        qpos, qvel, mocap = np.array([0.2, -0.2]), np.array([0.05, 0.0]), None
    return task, qpos, qvel, mocap


def oracle_derivatives(name, T):
    """A, B, cx, cu (last step without a transition) and the step times of an oracle rollout of a random cubic spline"""
    task, qpos, qvel, mocap = task_and_state(name)
    pm, pt = task.packed_model(differentiable=True), task.packed()
    nu, dt = pm.struct.nu, pm.struct.timestep
    times = np.linspace(0, max(T - 1, 1) * dt, 4)
    nodes = np.clip(np.random.default_rng(T).normal(0, 0.3, (1, 4, nu)), -1, 1)
    ref = pyoracle.rollout_batch(pm, pt, np.concatenate([qpos, qvel]), 0.0, mocap, 1, T, 4, 2, times, nodes, num_threads=4)
    nom = {k: v[0] for k, v in ref.items()}
    A, B, C, D = pyoracle.transition_fd(pm, pt, nom["states"], nom["times"], nom["actions"], 1e-5, 0, mocap=mocap, num_threads=8)
    A[T - 1] = 0; B[T - 1] = 0; D[T - 1] = 0
    cx, cu, _, _, _ = pyoracle.cost_derivatives(pt, nom["residual"], C, D)
    return pm, pt, A, B, cx, cu, nom["times"]


def close(a, b, tol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.all(np.abs(a - b) <= tol * (1 + np.abs(b)))


@pytest.mark.parametrize("T", [2, 36, 100])
@pytest.mark.parametrize("name", ["Particle", "Cartpole", "QuadrupedFlat"])
def test_gradient_pass_against_numpy(name, T):
    pm, pt, A, B, cx, cu, step_times = oracle_derivatives(name, T)
    ctx = capi.Context(pm, pt, 0, 64)
    if name == "QuadrupedFlat":
        assert A.shape[1] == 36 and B.shape[2] == 12 and "wave" in ctx.kernel_name
    for P in (1, 2, 5, 25):
        # node times as ResamplePolicy lays them out, shifted so that some step times fall on nodes and some outside
        shift = max((T - 1) * pm.struct.timestep / (P - 1), 1e-5) if P > 1 else 0.0
        nodes = 0.003 + np.arange(P) * shift
        for rep in (0, 1, 2):
            got = ctx.gradient_pass(A, B, cx, cu, rep, nodes, step_times)
            ref = gradient_pass(A, B, cx, cu, rep, nodes, step_times)
            for key in ("Vx", "k", "gradient"):
                assert close(got[key], ref[key], 1e-12), (P, rep, key, np.abs(got[key] - ref[key]).max())
            assert close(got["dV"][0], ref["dV"][0], 1e-12) and got["dV"][1] == 0
            assert got["kernel_ms"] > 0
    ctx.close()


def test_gradient_pass_limits(cartpole):
    ctx = capi.Context(cartpole.packed_model(), cartpole.packed(), 0, 64)
    rng = np.random.default_rng(0)

    def args(n, m, T, P):
        return (rng.normal(0, 0.2, (T, n, n)), rng.normal(0, 1, (T, n, m)), rng.normal(0, 1, (T, n)), rng.normal(0, 1, (T, m)), 2,
                np.linspace(0, 0.1, P) if P > 1 else [0.0], 0.1 * np.arange(T) / max(T - 1, 1))
    a = args(48, 16, 20, 25)                       # the largest sizes the kernel covers
    got, ref = ctx.gradient_pass(*a), gradient_pass(*a)
    for key in ("Vx", "k", "gradient"):
        assert close(got[key], ref[key], 1e-12)
    for (n, m, T, P), code in (((49, 4, 10, 5), -2), ((8, 17, 10, 5), -2), ((8, 4, 1, 5), -1), ((8, 4, 10, 26), -2)):
        with pytest.raises(capi.MjpcxError) as e:
            ctx.gradient_pass(*args(n, m, T, P))
        assert e.value.code == code and "gradient pass" in str(e.value)
    A, B, cx, cu, _, nodes, times = args(4, 2, 10, 3)
    with pytest.raises(capi.MjpcxError) as e:
        ctx.gradient_pass(A, B, cx, cu, 3, nodes, times)
    assert e.value.code == -1
    with pytest.raises(capi.MjpcxError) as e:
        ctx.gradient_pass(A, B, cx, cu, 1, [0.0, 0.1, 0.1], times)
    assert e.value.code == -1 and "increasing" in str(e.value)
    ctx.close()


def resampled(task, times, values, rep, time, H):
    """ResamplePolicy (planner.cc:355-381) of the spline (times, values) at `time` with the Python policy"""
    pol = GradientPolicy(task.model, task)
    P = len(times)
    pol.num_spline_points, pol.representation = P, rep
    pol.times[:P], pol.parameters[:P] = times, values
    shift = max((H - 1) * task.model.get_number("agent_timestep", task.model.timestep) / (P - 1), 1e-5) if P > 1 else 0.0
    theta, t = np.zeros((P, task.model.nu)), time
    for i in range(P):
        pol.action(theta[i], None, t)
        t += shift
    return theta, time + np.arange(P) * shift


@pytest.mark.parametrize("rep", [0, 1, 2])
def test_line_search_actions(rep):
    """every candidate of one C++ iteration on Cartpole: the actions the device applied are clamp(interp(theta + s_i g))"""
    from mujoco_mpc_amd.hostplanner import HostPlanner
    task, qpos, qvel, _ = task_and_state("Cartpole")
    H, N = 36, 32
    cpp = HostPlanner(task, kind="gradient", num_trajectory=N)
    cpp.reset(H)
    cpp.gradient_set(representation=rep)
    cpp.set_state(qpos, qvel, 0.0)
    cpp.optimize_policy(H)
    times, values = cpp.policy()
    cpp.set_state(qpos, qvel, 0.02)
    cpp.optimize_policy(H)
    res = cpp.gradient_result()
    theta, node_times = resampled(task, times, values, rep, 0.02, H)
    steps = np.concatenate([log_scale(1.0, 1e-8, N - 1), [0.0]])
    pol = GradientPolicy(task.model, task)
    pol.num_spline_points, pol.representation = len(times), rep
    pol.times[:len(times)] = node_times
    assert np.abs(res["gradient"]).max() > 0
    for i in range(N):
        pol.parameters[:len(times)] = theta + steps[i] * res["gradient"]
        tr = cpp.fetch_trajectory(i, H)
        want = np.array([pol.action(np.zeros(1), None, t) for t in tr.times[:H - 1]])
        np.testing.assert_allclose(tr.actions[:H - 1], want, rtol=0, atol=1e-12)
        np.testing.assert_array_equal(tr.actions[H - 1], tr.actions[H - 2])
    cpp.close()


@pytest.mark.parametrize("skip", [0, 3])
@pytest.mark.parametrize("name", ["Cartpole", "QuadrupedFlat"])
def test_cpp_planner_matches_python_mirror_on_oracle(name, skip):
    from mujoco_mpc_amd.hostplanner import HostPlanner
    task, qpos, qvel, mocap = task_and_state(name)
    H, N = 36, 32
    cpp = HostPlanner(task_and_state(name)[0], kind="gradient", num_trajectory=N)
    if name == "QuadrupedFlat":
        cpp.task_transition(0.0)
    cpp.reset(H)
    cpp.gradient_set(derivative_skip=skip)
    py = GpuGradientPlanner(backend_factory=lambda t: OracleGradientContext(t, threads=8, differentiable=True))
    py.initialize(task.model, task); py.num_trajectory = N; py.allocate(); py.reset(H)
    py.derivative_skip_ = skip
    st = State(task.model)
    if mocap is None:
        st.set(qpos, qvel, time=0.0)
        cpp.set_state(qpos, qvel, 0.0)
    else:
        st.set(qpos, qvel, mocap_pos=QUAD_MOCAP_POS, mocap_quat=QUAD_MOCAP_QUAT, time=0.0)
        cpp.set_state(qpos, qvel, 0.0, mocap_pos=QUAD_MOCAP_POS, mocap_quat=QUAD_MOCAP_QUAT)
    py.set_state(st)
    py.optimize_policy(H)
    cpp.optimize_policy(H)
    res = cpp.gradient_result()
    P = py.policy.num_spline_points
    rel = lambda a, b: np.all(np.abs(np.asarray(a) - b) <= 1e-7 * np.maximum(1.0, np.abs(b)))
    assert res["winner"] == py.winner and res["action_step"] == py.action_step
    ct, cv = cpp.policy()
    np.testing.assert_array_equal(ct, py.policy.times[:P])
    assert rel(cv, py.policy.parameters[:P]), np.abs(cv - py.policy.parameters[:P]).max()
    assert rel(res["gradient"], py.candidate0.parameter_update[:P])
    assert rel(res["expected"], py.expected) and rel(res["improvement"], py.improvement)
    assert py.improvement > 0
    if name == "QuadrupedFlat" and skip == 0:
        print("gradient planner stage times [us], QuadrupedFlat T=36 N=32 fp64:", cpp.gradient_timers())
    cpp.close()


def test_particle_behaviour():
    """20 iterations from far from the goal: winners never worse than their nominal, the nominal return falls by >= 10 %, and
    an iteration whose only candidate is the zero step leaves the resampled policy bit for bit"""
    from mujoco_mpc_amd.hostplanner import HostPlanner
    task, _, _, _ = task_and_state("Particle")
    H = task.planning_steps()
    cpp = HostPlanner(task, kind="gradient")
    cpp.reset(H)
    qpos, qvel = np.array([0.25, -0.25]), np.zeros(2)
    nominal = []
    for _ in range(20):
        cpp.set_state(qpos, qvel, 0.0)
        cpp.optimize_policy(H)
        res = cpp.gradient_result()
        best = cpp.best_trajectory()["total_return"]
        assert res["improvement"] >= 0
        nominal.append(best + res["improvement"])
    assert nominal[-1] <= 0.9 * nominal[0], nominal
    times, values = cpp.policy()
    theta, node_times = resampled(task, times, values, 1, 0.0, H)
    cpp.gradient_set(num_trajectory=1)
    cpp.set_state(qpos, qvel, 0.0)
    cpp.optimize_policy(H)
    res = cpp.gradient_result()
    assert res["winner"] == 0 and res["action_step"] == 0 and res["improvement"] == 0
    t2, v2 = cpp.policy()
    np.testing.assert_array_equal(t2, node_times)
    np.testing.assert_array_equal(v2, theta)
    cpp.close()


def test_fp32_wave_family_is_refused():
    """the iLQG kernels of the wavefront-per-candidate family are fp64 only: an fp32 planner on the A1 fails with the library's
    message instead of returning a policy"""
    from mujoco_mpc_amd.hostplanner import HostPlanner
    task, qpos, qvel, _ = task_and_state("QuadrupedFlat")
    try:
        cpp = HostPlanner(task, kind="gradient", precision=32, num_trajectory=8)
    except RuntimeError as e:
        assert "fp64 only" in str(e)
        return
    cpp.task_transition(0.0)
    cpp.reset(12)
    cpp.set_state(qpos, qvel, 0.0, mocap_pos=QUAD_MOCAP_POS, mocap_quat=QUAD_MOCAP_QUAT)
    before = cpp.policy()
    with pytest.raises(RuntimeError, match="fp64 only"):
        cpp.optimize_policy(12)
    after = cpp.policy()
    np.testing.assert_array_equal(before[1], after[1])
    cpp.close()
