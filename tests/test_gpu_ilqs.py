"""-m gpu: the iLQS planner on the device.
   mjpc::GpuILQSPlanner (C++, GPU) <-> planners.GpuILQSPlanner on the oracle backend          1e-7 relative
   the iLQG -> sampling conversion <-> mjpc_ilqs_fit_spline, and candidate 0 of the next launch  1e-12
The first is looser for the reason tests/test_gpu_gradient.py gives: the device's and the oracle's finite-difference
derivatives differ by about 1e-9 absolute."""
import numpy as np
import pytest

from mujoco_mpc_amd import capi
from mujoco_mpc_amd.cstructs import as_f64p
from mujoco_mpc_amd.planners import GpuILQSPlanner, State
from mujoco_mpc_amd.spline import TimeSpline
from oracle_backend import OracleContext

pytestmark = pytest.mark.gpu

QUAD_MOCAP_POS = np.array([[0.3, 0, 0.26], [-2.5, 0, 0]])
QUAD_MOCAP_QUAT = np.array([[1.0, 0, 0, 0], [1.0, 0, 0, 0]])
H, N = 36, 32


def load(name):
    from mujoco_mpc_amd.task import load_task
    task = load_task(name)
    if name == "QuadrupedFlat":
        task.transition(0.0)
    return task


def state_at(task, name, k):
    """the state of plan k: every third plan starts from a pushed state, so that sampling can win back from iLQG"""
    rng = np.random.default_rng(1000 + k)
    push = k % 3 == 2
    if name == "Cartpole":
        return np.array([0.3, 2.5]) + rng.normal(0, 0.3, 2) * push, np.array([-0.2, 0.4])
    qvel = np.zeros(18)
    qvel[:6] += rng.normal(0, 0.5, 6) * push
    return task.model.keyframes["home"]["qpos"].copy(), qvel


def set_state(name, cpp, py, st, q, v, t):
    if name == "QuadrupedFlat":
        st.set(q, v, mocap_pos=QUAD_MOCAP_POS, mocap_quat=QUAD_MOCAP_QUAT, time=t)
        cpp.set_state(q, v, t, mocap_pos=QUAD_MOCAP_POS, mocap_quat=QUAD_MOCAP_QUAT)
    else:
        st.set(q, v, time=t)
        cpp.set_state(q, v, t)
    if py is not None:
        py.set_state(st)


def rel(a, b, tol=1e-7):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b)))


SEEDS = {"Cartpole": 0, "QuadrupedFlat": 5}   # each switches both ways within 8 plans (asserted below)


@pytest.mark.parametrize("name", ["Cartpole", "QuadrupedFlat"])
def test_cpp_planner_matches_python_mirror_on_oracle(name):
    from mujoco_mpc_amd.hostplanner import HostPlanner
    task = load(name)
    seed = SEEDS[name]
    cpp = HostPlanner(load(name), kind="ilqs", seed=seed, num_trajectory=N)
    if name == "QuadrupedFlat":
        cpp.task_transition(0.0)
    cpp.reset(H)
    py = GpuILQSPlanner(seed=seed, backend_factory=lambda t: OracleContext(t, threads=8, differentiable=True))
    py.initialize(task.model, task)
    py.sampling.num_trajectory_ = N
    py.allocate()
    py.reset(H)
    st = State(task.model)
    switches = set()
    for k in range(8):
        q, v = state_at(task, name, k)
        set_state(name, cpp, py, st, q, v, 0.01 * k)
        py.optimize_policy(H)
        cpp.optimize_policy(H)
        info = cpp.ilqs_info()
        # a winner flip between two candidates closer than this would be a tie, not a defect
        r = np.sort(py.sampling.ctx.returns()[0])
        assert r[1] - r[0] > 1e-6 * abs(r[0]), (k, r[:2])
        want = dict(active=py.active_policy, previous_active=py.previous_active_policy, ilqg_ran=int(py.ilqg_ran),
                    sampling_winner=py.sampling.winner, fit_status=py.fit_status, fit_unreached=py.fit_unreached)
        assert {key: info[key] for key in want} == want, (k, info)
        assert rel(info["sampling_best_return"], py.sampling.best_return)
        assert rel(info["sampling_nominal_return"], py.sampling.nominal_return)
        if py.ilqg_ran:
            assert info["iteration_completed"] == int(py.ilqg.iteration_completed) and info["ilqg_winner"] == py.ilqg.winner
            assert rel(info["ilqg_winner_return"], py.ilqg.winner_return)
            assert rel(info["ilqg_linesearch0_return"], py.ilqg.linesearch0_return)
        ct, cv = cpp.policy()
        np.testing.assert_array_equal(ct, py.sampling.policy.plan.times())
        assert rel(cv, py.sampling.policy.plan.values())
        for t in 0.01 * k + np.linspace(0.0, 0.3, 5):
            for previous in (False, True):
                want_a = py.action_from_policy(np.zeros(task.model.nu), None, t, previous)
                assert rel(cpp.action(t, use_previous=previous), want_a), (k, t, previous)
        switches.add((info["previous_active"], info["active"]))
        if name == "QuadrupedFlat":
            print(f"iLQS stage times [us], QuadrupedFlat T={H} N={N} fp64, plan {k}:",
                  {key: info[key] for key in ("nominal_us", "fit_us", "sampling_us", "handoff_us", "iteration_us")},
                  "active:", info["active"])
    assert (0, 1) in switches and (1, 0) in switches, switches   # the seed switches both ways
    cpp.close()


def run_until_ilqg_active(cpp, task, name, limit=8):
    st = State(task.model)
    for k in range(limit):
        q, v = state_at(task, name, k)
        set_state(name, cpp, None, st, q, v, 0.01 * k)
        cpp.optimize_policy(H)
        if cpp.ilqs_info()["active"] == 1:
            return k
    pytest.fail("iLQG never became active")


def test_conversion_on_the_device():
    """after a plan that ends with iLQG active, the next plan's fit is mjpc_ilqs_fit_spline of the actions it recorded, and
    candidate 0 of its sampling launch applies exactly that spline"""
    from mujoco_mpc_amd.hostplanner import HostPlanner, ilqs_fit_spline
    name = "Cartpole"
    task = load(name)
    cpp = HostPlanner(task, kind="ilqs", seed=SEEDS[name], num_trajectory=N)
    cpp.reset(H)
    k = run_until_ilqg_active(cpp, task, name)
    q, v = state_at(task, name, 0)
    cpp.set_state(q, v, 0.01 * (k + 1))
    cpp.optimize_policy(H)
    info = cpp.ilqs_info()
    assert info["previous_active"] == 1 and info["fit_status"] == 0
    fit = cpp.ilqs_last_fit()
    assert len(fit["step_times"]) == H - 1 and fit["node_times"][0] == 0.01 * (k + 1)
    want, status, _ = ilqs_fit_spline(2, fit["node_times"], fit["step_times"], fit["actions"], task.model.actuator_ctrlrange)
    assert status == 0
    np.testing.assert_allclose(fit["values"], want, rtol=0, atol=1e-12)
    tr = cpp.fetch_trajectory(0, H)
    spline = TimeSpline(task.model.nu, 2)
    for t, x in zip(fit["node_times"], fit["values"]):
        spline.add_node(t, x)
    bounds = np.asarray(task.model.actuator_ctrlrange, float).reshape(-1, 2)
    applied = np.array([np.clip(spline.sample(t), bounds[:, 0], bounds[:, 1]) for t in tr.times[:H - 1]])
    np.testing.assert_allclose(tr.actions[:H - 1], applied, rtol=0, atol=1e-12)
    cpp.close()


def test_both_halves_plan_on_one_model():
    """after a sampling -> iLQG handoff (one sampling candidate: sampling never wins), sampling's candidate 0 has the return its
    spline has on a context of the differentiable model -- the model the iLQG half plans on"""
    from mujoco_mpc_amd.hostplanner import HostPlanner
    name = "QuadrupedFlat"
    task = load(name)
    cpp = HostPlanner(load(name), kind="ilqs", num_trajectory=1)
    cpp.task_transition(0.0)
    cpp.reset(H)
    st = State(task.model)
    q, v = state_at(task, name, 0)
    set_state(name, cpp, None, st, q, v, 0.0)
    cpp.optimize_policy(H)
    info = cpp.ilqs_info()
    assert info["previous_active"] == 0 and info["ilqg_ran"] == 1   # the handoff happened
    t_nodes, _ = cpp.policy()                                         # the launch's node times (its winner is candidate 0)
    nodes = np.zeros((len(t_nodes), task.model.nu))
    assert capi.lib().mjpcx_fetch_spline(cpp._ctx(), 0, as_f64p(nodes)) == 0
    tr = cpp.fetch_trajectory(0, H)
    ctx = capi.Context(task.packed_model(differentiable=True), task.packed(), 0, 64)
    ctx.set_state(np.concatenate([q, v]), 0.0, np.concatenate([np.concatenate([p, r]) for p, r in zip(QUAD_MOCAP_POS, QUAD_MOCAP_QUAT)]))
    ctx.rollout_splines(H, 2, t_nodes, nodes[None])
    assert abs(ctx.returns()[0][0] - tr.total_return) <= 1e-9 * (1 + abs(tr.total_return))
    assert abs(info["sampling_nominal_return"] - tr.total_return) <= 1e-9 * (1 + abs(tr.total_return))
    ctx.close()
    cpp.close()


def test_one_sample_is_ilqg():
    from mujoco_mpc_amd.hostplanner import HostPlanner
    task = load("Cartpole")
    ilqs = HostPlanner(task, kind="ilqs", num_trajectory=1)
    ilqg = HostPlanner(task, kind="ilqg")
    for p in (ilqs, ilqg):
        p.reset(H)
    for k in range(5):
        for p in (ilqs, ilqg):
            p.set_state([0.3, 2.5], [-0.2, 0.4], 0.01 * k)
            p.optimize_policy(H)
        assert ilqs.ilqs_info()["active"] == 1
        for a, b in zip(ilqs.ilqg_policy(H), ilqg.ilqg_policy(H)):
            assert np.all(np.abs(a - b) <= 1e-9 * (1 + np.abs(b)))
    ilqs.close()
    ilqg.close()


def test_refusals():
    """fp32 on the A1: the iLQG half's kernels are fp64 only. One sampling candidate makes the iLQG half run after the sampling
    launch, and the failed plan leaves the policy as it was."""
    from mujoco_mpc_amd.hostplanner import HostPlanner, comm_unique_id
    task = load("QuadrupedFlat")
    try:
        cpp = HostPlanner(task, kind="ilqs", precision=32, num_trajectory=1)
    except RuntimeError as e:
        assert "fp64 only" in str(e)
    else:
        cpp.task_transition(0.0)
        cpp.reset(12)
        cpp.set_state(task.model.keyframes["home"]["qpos"], np.zeros(18), 0.0, mocap_pos=QUAD_MOCAP_POS, mocap_quat=QUAD_MOCAP_QUAT)
        before = cpp.policy()
        with pytest.raises(RuntimeError, match="fp64 only"):
            cpp.optimize_policy(12)
        after = cpp.policy()
        np.testing.assert_array_equal(before[0], after[0])
        np.testing.assert_array_equal(before[1], after[1])
        cpp.close()
    with pytest.raises(RuntimeError, match="the ilqs planner is not sharded \\(replicas only\\)"):
        HostPlanner(load("Cartpole"), kind="ilqs", native_comm=(comm_unique_id(), 0, 1))
