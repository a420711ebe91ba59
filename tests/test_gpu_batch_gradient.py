"""-m gpu: the Gradient planner's derivative chain for a fleet (mjpcx_gradient_step_batched) and GpuBatchGradientPlanner on the device.

   mjpcx_gradient_step_batched <-> mjpcx_transition_fd -> numpy interpolation and zeroing -> mjpcx_cost_derivatives ->
       mjpcx_gradient_pass, fed with mjpcx_fetch_trajectory of the same batched rollout:
         every step evaluated (skip 0)   bit for bit: every item does the same arithmetic on the same inputs in the same kernels
         derivative_skip 3               1e-12 (1 + |x|), tests/test_gpu_gradient.py's bound for the gradient pass (the device
                                         interpolation is not contracted, so equality is the expected outcome; the maximum is printed)
   permuting the environments permutes the outputs bit for bit; two calls on one rollout give the same bits
   GpuBatchGradientPlanner on the GPU <-> the same planner on the oracle backend: equal winners; parameters, dV and returns to
       1e-7 max(1, |x|), tests/test_gpu_gradient.py's figure for this pair (the two sides' finite differences differ by ~1e-9)
The sharded-context refusal (world > 1) needs two ranks and is not exercised here."""
import numpy as np
import pytest

import step_bank
from batch_gradient_oracle_backend import BatchGradientOracleContext, interpolate
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import GpuBatchGradientPlanner, State, derivative_steps
from mujoco_mpc_amd.task import load_task

pytestmark = pytest.mark.gpu

E, N, H, T, P = 4, 64, 24, 20, 5
MATRICES = ("A", "B", "cx", "cu")
RESULTS = ("nominal_return", "k", "gradient", "dV")


class Env:
    def __init__(self, state, time, mocap, residual_int=(), residual_real=()):
        self.state, self.time, self.mocap = np.asarray(state, float), float(time), mocap
        self.residual_int, self.residual_real = list(residual_int), list(residual_real)


def fleet(name, per_env_residual=False):
    """the task and four environments with different states, clocks and mocap poses (the A1: from tests/step_bank.py, home and the trot)"""
    rng = np.random.default_rng(23)
    if name == "QuadrupedFlat":
        bank = step_bank.a1_bank()
        task, envs = bank.task, []
        for e in range(E):
            s = bank.states[e]                                      # home/mode0, trot0/mode1, trot1/mode2, trot2/mode3
            mocap = np.array([0.3 + 0.2 * e, -0.1 * e, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])
            r = s if per_env_residual else bank.states[0]
            envs.append(Env(s.state, s.time, mocap, r.residual_int, r.residual_real))
        return task, envs
    task = load_task(name)
    m = task.model
    envs = []
    for e in range(E):
        q = rng.uniform(-0.5, 0.5, m.nq) * (1.0 if name == "Cartpole" else 0.2)
        v = rng.normal(0, 0.3, m.nv)
        mocap = np.array([0.1 * (e + 1), -0.05 * e, 0.01, 1, 0, 0, 0]) if m.nmocap else None
        envs.append(Env(np.concatenate([q, v]), 0.1 * e, mocap))
    return task, envs


def plan_inputs(task, envs, horizon=H, num_nodes=P):
    m = task.model
    dt = m.get_number("agent_timestep", m.timestep)
    times = np.stack([s.time + np.arange(num_nodes) * ((horizon - 1) * dt / max(num_nodes - 1, 1)) for s in envs])
    lo, hi = np.asarray(m.arrays["actuator_ctrlrange"], float).reshape(-1, 2).T
    nodes = np.clip(np.random.default_rng(7).normal(0, 0.2, (len(envs), N, num_nodes, m.nu)), lo, hi)
    return times, nodes


def make_context(task, envs, precision=64):
    return capi.Context(task.packed_model(differentiable=True), step_bank.packed_task(task, envs[0]), 0, precision)


def rollout_batched(ctx, task, envs, times, nodes, per_env_residual=False, horizon=H, interp=capi.SPLINE_LINEAR):
    ctx.set_states(np.stack([s.state for s in envs]), [s.time for s in envs], np.stack([s.mocap for s in envs]) if task.model.nmocap else None)
    if per_env_residual:
        ctx.set_residual_states(np.array([s.residual_int for s in envs], np.int32), np.array([s.residual_real for s in envs], float))
    elif envs[0].residual_int or envs[0].residual_real:
        ctx.set_residual_state(envs[0].residual_int, envs[0].residual_real)
    ctx.rollout_splines_batched(horizon, interp, times, nodes, num_envs=len(envs), n_per_env=N)


def sequential_chain(ctx, task, env, tr, ev, eps, centered, rep, node_times):
    """the four plain calls of one GpuGradientPlanner step on environment `env`, fed with its fetched nominal trajectory"""
    if env.residual_int or env.residual_real:
        ctx.set_residual_state(env.residual_int, env.residual_real)
    ctx.set_state(env.state, env.time, env.mocap if task.model.nmocap else None)
    A, B, C, D = interpolate(ev, T, ctx.transition_fd(tr.times[ev], tr.states[ev], tr.actions[ev], eps, centered))
    A[T - 1] = 0; B[T - 1] = 0; D[T - 1] = 0
    cx, cu, _, _, _ = ctx.cost_derivatives(tr.residual[:T], np.asarray(C), np.asarray(D))
    out = ctx.gradient_pass(np.asarray(A), np.asarray(B), cx, cu, rep, node_times, tr.times[:T])
    return dict(nominal_return=tr.total_return, k=out["k"], gradient=out["gradient"], dV=out["dV"], A=A, B=B, cx=cx, cu=cu)


def compare_with_chain(name, candidate, centered, skip, precision=64, per_env_residual=False, rep=2):
    task, envs = fleet(name, per_env_residual)
    ctx = make_context(task, envs, precision)
    times, nodes = plan_inputs(task, envs)
    rollout_batched(ctx, task, envs, times, nodes, per_env_residual)
    _, fail = ctx.returns()
    assert not fail.reshape(E, N)[:, candidate].any()
    trs = [ctx.fetch_trajectory(e * N + candidate) for e in range(E)]
    ev = derivative_steps(T, skip)
    assert (len(ev) == T) == (skip == 0)
    eps = 1e-5
    got = ctx.gradient_step_batched(E, candidate, T, ev, eps, centered, rep, times, with_matrices=True)
    again = ctx.gradient_step_batched(E, candidate, T, ev, eps, centered, rep, times, with_matrices=True)
    for key in RESULTS + MATRICES:                                   # deterministic: the same bits from the same rollout
        assert np.array_equal(got[key], again[key]), key
    worst = 0.0
    for e in range(E):
        ref = sequential_chain(ctx, task, envs[e], trs[e], ev, eps, centered, rep, times[e])
        for key in RESULTS + MATRICES:
            g, r = np.asarray(got[key][e], float), np.asarray(ref[key], float)
            assert np.all(np.isfinite(r)), (e, key)
            if skip == 0:
                assert np.array_equal(g, r), (name, e, key, float(np.abs(g - r).max()))
            else:
                err = float(np.max(np.abs(g - r) / (1 + np.abs(r))))
                worst = max(worst, err)
                assert err <= 1e-12, (name, e, key, err)
        assert np.abs(got["gradient"][e]).max() > 0 and got["dV"][e][0] < 0 and got["dV"][e][1] == 0
    if skip:
        print(f"gradient_step_batched vs sequential chain, {name} skip {skip} candidate {candidate} centered {centered}: max err {worst:.3e}")
    # the environments are different problems
    assert len({tuple(np.round(got["gradient"][e].ravel(), 12)) for e in range(E)}) == E
    ctx.close()


@pytest.mark.parametrize("skip", [0, 3])
@pytest.mark.parametrize("centered", [0, 1])
@pytest.mark.parametrize("candidate", [0, 5])
@pytest.mark.parametrize("name", ["Cartpole", "Particle", "QuadrupedFlat"])
def test_batched_step_equals_the_sequential_chain(name, candidate, centered, skip):
    compare_with_chain(name, candidate, centered, skip)


@pytest.mark.parametrize("skip", [0, 3])
def test_per_environment_residual_state(skip):
    """four Quadruped modes in one fleet (set_residual_states): every environment's finite differences read its own frozen state"""
    task, envs = fleet("QuadrupedFlat", per_env_residual=True)
    assert len({s.residual_int[0] for s in envs}) == E
    compare_with_chain("QuadrupedFlat", 5, 0, skip, per_env_residual=True)


@pytest.mark.parametrize("name", ["Cartpole", "Particle"])
def test_fp32_lane_contexts(name):
    """fp32 contexts of the lane family work: finite differences in fp32, the rest in fp64, as the plain calls -- the same equality"""
    compare_with_chain(name, 5, 0, 0, precision=32)
    compare_with_chain(name, 0, 1, 3, precision=32)


@pytest.mark.parametrize("name", ["Particle", "QuadrupedFlat"])
def test_environment_independence(name):
    """permuting the environments' states permutes the outputs bit for bit"""
    per_env = name == "QuadrupedFlat"
    task, envs = fleet(name, per_env)
    times, nodes = plan_inputs(task, envs)
    ev = derivative_steps(T, 0)
    ctx = make_context(task, envs)
    rollout_batched(ctx, task, envs, times, nodes, per_env)
    base = ctx.gradient_step_batched(E, 5, T, ev, 1e-5, 0, 1, times, with_matrices=True)
    perm = [2, 0, 3, 1]
    rollout_batched(ctx, task, [envs[i] for i in perm], times[perm], nodes[perm], per_env)
    got = ctx.gradient_step_batched(E, 5, T, ev, 1e-5, 0, 1, times[perm], with_matrices=True)
    for key in RESULTS + MATRICES:
        assert np.array_equal(got[key], base[key][perm]), key
    ctx.close()


def test_argument_checks():
    task, envs = fleet("Cartpole")
    ctx = make_context(task, envs)
    times, nodes = plan_inputs(task, envs)
    ev = derivative_steps(T, 0)

    def call(num_envs=E, candidate=0, steps=T, evaluate=ev, eps=1e-5, rep=1, node_times=times):
        return ctx.gradient_step_batched(num_envs, candidate, steps, evaluate, eps, 0, rep, node_times)

    def refused(code, match, **kw):
        with pytest.raises(capi.MjpcxError, match=match) as e:
            call(**kw)
        assert e.value.code == code, (kw, e.value.code)

    ctx.set_state(envs[0].state, envs[0].time)
    ctx.rollout_splines(H, capi.SPLINE_LINEAR, times[0], nodes[0])
    refused(-1, "not a batched one")                                  # the last rollout was a plain one
    rollout_batched(ctx, task, envs, times, nodes)
    call()
    refused(-1, "not a batched one", num_envs=2, node_times=times[:2])
    refused(-1, "candidate", candidate=-1)
    refused(-1, "candidate", candidate=N)
    refused(-1, "horizon", steps=1, evaluate=[0])
    refused(-1, "horizon", steps=H + 1, evaluate=derivative_steps(H + 1, 0))
    refused(-1, "evaluate", evaluate=[0, 5, 5, T - 1])
    refused(-1, "evaluate", evaluate=[0, 7, 3, T - 1])
    refused(-1, "evaluate", evaluate=[0, T])
    refused(-1, "evaluate", evaluate=[-1, 3])
    refused(-1, "num_eval", evaluate=[])
    refused(-1, "epsilon", eps=0.0)
    refused(-1, "representation", rep=3)
    bad = times.copy()
    bad[2, 3] = bad[2, 2]
    refused(-1, "increasing", node_times=bad)
    # beyond the kernels' limits: P = 26 spline points, T = 513 steps
    for horizon, num_nodes, steps in ((H, 26, T), (513, P, 513)):
        t2, n2 = plan_inputs(task, envs, horizon, num_nodes)
        rollout_batched(ctx, task, envs, t2, n2, horizon=horizon)
        refused(-2, "covers", steps=steps, evaluate=derivative_steps(steps, 0), node_times=t2)
    ctx.close()


def test_fp32_wave_family_is_refused():
    """as mjpcx_transition_fd: the finite-difference kernels of the wavefront-per-candidate family are fp64 only"""
    task, envs = fleet("QuadrupedFlat")
    ctx = make_context(task, envs, precision=32)
    times, nodes = plan_inputs(task, envs)
    rollout_batched(ctx, task, envs, times, nodes)
    with pytest.raises(capi.MjpcxError, match="fp64 only") as e:
        ctx.gradient_step_batched(E, 0, T, derivative_steps(T, 0), 1e-5, 0, 1, times)
    assert e.value.code == -2
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- the planner
def planner_fleet(name):
    task, envs = fleet(name)
    states = []
    for s in envs[:3]:
        st = State(task.model)
        nq = task.model.nq
        mp = None if s.mocap is None else s.mocap.reshape(-1, 7)
        st.set(s.state[:nq], s.state[nq:], mocap_pos=None if mp is None else mp[:, :3], mocap_quat=None if mp is None else mp[:, 3:], time=s.time)
        states.append(st)
    if name == "QuadrupedFlat":
        task = load_task(name)
        task.transition(0.0)
    return task, states


def planner(task, H, skip, backend_factory=None):
    p = GpuBatchGradientPlanner(3, backend_factory=backend_factory)
    p.initialize(task.model, task)
    p.num_trajectory = N
    p.allocate()
    p.reset(H)
    p.derivative_skip_ = skip
    return p


@pytest.mark.parametrize("skip", [0, 3])
@pytest.mark.parametrize("name", ["Cartpole", "QuadrupedFlat"])
def test_planner_matches_the_oracle_backend(name, skip):
    task, states = planner_fleet(name)
    horizon = 36
    gpu = planner(task, horizon, skip)
    ora = planner(task, horizon, skip, lambda t: BatchGradientOracleContext(t, threads=8, differentiable=True))
    for p in (gpu, ora):
        p.set_states(states)
        p.optimize_policy(horizon)
    rel = lambda a, b: np.all(np.abs(np.asarray(a, float) - np.asarray(b, float)) <= 1e-7 * np.maximum(1.0, np.abs(np.asarray(b, float))))
    # a near tie on the oracle side could flip the winner: its two best line-search returns are more than 1e-6 (relative) apart
    ret = ora.ctx.out["total_return"].reshape(3, N)
    for e in range(3):
        r = np.sort(ret[e][ora.ctx.out["failure"].reshape(3, N)[e] == 0])
        assert (r[1] - r[0]) > 1e-6 * max(1.0, abs(r[0])), (e, r[:3])
        assert ora.envs[e].improvement > 0
    P_ = ora.envs[0].policy.num_spline_points
    for e, (g, o) in enumerate(zip(gpu.envs, ora.envs)):
        assert g.winner == o.winner and g.action_step == o.action_step, (e, g.winner, o.winner)
        np.testing.assert_array_equal(g.policy.times[:P_], o.policy.times[:P_])
        assert rel(g.policy.parameters[:P_], o.policy.parameters[:P_]), (e, np.abs(g.policy.parameters[:P_] - o.policy.parameters[:P_]).max())
        assert rel(g.candidate0.parameter_update[:P_], o.candidate0.parameter_update[:P_]), e
        assert rel(g.dV, o.dV), (e, g.dV, o.dV)
        assert rel(g.improvement, o.improvement) and rel(g.expected, o.expected), e
        assert rel(gpu.best_trajectory(e).total_return, ora.best_trajectory(e).total_return), e
    gpu.ctx.close()
