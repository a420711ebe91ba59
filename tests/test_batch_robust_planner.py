"""GpuRobustPlanner and GpuBatchRobustPlanner (mujoco_mpc_amd/planners.py) on the oracle-backed test backend
(batch_robust_oracle_backend.py): the Robust planner for E robots on two contexts is, robot by robot, GpuRobustPlanner over
GpuSamplingPlanner with seed s + e. Both sides run the oracle, so equality is exact."""
import os
import re

import numpy as np
import pytest

import task_rows
from batch_robust_oracle_backend import BatchRobustOracleContext
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import GpuBatchRobustPlanner, GpuBatchSamplingPlanner, GpuRobustPlanner, GpuSamplingPlanner, State, robust_scores
from mujoco_mpc_amd.task import load_task

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, STEPS, SEED, N = 3, 3, 9, 64
PAIRS = [(5, 4), (13, 5), (16, 4)]   # k x R = 20, 65, 64 perturbed rollouts: the padding to 64 below, across and exactly on a boundary
HORIZON = {"Cartpole": 20, "Particle": 12, "QuadrupedFlat": 10}


def test_the_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mjpcx.h")).read(), flags=re.S)
    for name, method in (("mjpcx_rollout_splines_noisy_batched", "rollout_splines_noisy_batched"), ("mjpcx_robust_step_batched", "robust_step_batched")):
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert name in capi.EXPORTS
        assert hasattr(capi.lib(), name) and getattr(capi.lib(), name).argtypes is not None
        assert callable(getattr(capi.Context, method))


def backend(task):
    return BatchRobustOracleContext(task, threads=8)


def configure(p, task, k, R, xfrc_std=None, n=N):
    p.initialize(task.model, task)
    for q in (p.envs if hasattr(p, "envs") else [p]):
        q.ncandidates_, q.nrepetitions_ = k, R
        if xfrc_std is not None:
            q.xfrc_std_ = xfrc_std
        q.delegate.num_trajectory_ = n
        if task.name == "QuadrupedFlat":
            q.delegate.noise_exploration = [0.05, 0.0]
            q.xfrc_std_ = 0.3 if xfrc_std is None else xfrc_std
    p.allocate()
    return p


def fleet_planner(task, k, R, xfrc_std=None, tasks=None, seed=SEED, factory=backend):
    p = configure(GpuBatchRobustPlanner(E, seed=seed, backend_factory=factory), task, k, R, xfrc_std)
    if tasks is not None:
        p.set_tasks(tasks)
    return p


def single_planner(task, seed, k, R, xfrc_std=None, factory=backend):
    return configure(GpuRobustPlanner(GpuSamplingPlanner(seed=seed, backend_factory=factory), seed=seed, backend_factory=factory), task, k, R, xfrc_std)


def initial_states(task, zero=False):
    """three different states (or three times the zero state); a different mocap goal per environment"""
    m = task.model
    rng = np.random.default_rng(17)
    out = []
    for e in range(E):
        st = State(m)
        if task.name == "QuadrupedFlat":
            q = np.asarray(m.keyframes["home"]["qpos"], float).copy()
            q[7:] += rng.normal(0, 0.05, 12)
            st.set(q, rng.normal(0, 0.1, 18), mocap_pos=[[0.3 + 0.1 * e, -0.1 * e, 0.26], [-2.5, 0, 0]], mocap_quat=[[1, 0, 0, 0], [1, 0, 0, 0]], time=0.04 * e)
        else:
            q = np.zeros(m.nq) if zero else rng.uniform(-0.5, 0.5, m.nq) * (1.0 if task.name == "Cartpole" else 0.2)
            v = np.zeros(m.nv) if zero else rng.normal(0, 0.3, m.nv)
            if m.nmocap:
                st.set(q, v, mocap_pos=[[0.1 * (e + 1), -0.05 * e, 0.01]], mocap_quat=[[1, 0, 0, 0]], time=0.1 * e)
            else:
                st.set(q, v, time=0.1 * e)
        out.append(st)
    return out


def step_along(task, states, singles):
    nq = task.model.nq
    for e in range(E):
        tr = singles[e].best_trajectory()
        mp = states[e].mocap.reshape(-1, 7)
        states[e].set(tr.states[2, :nq], tr.states[2, nq:], mocap_pos=mp[:, :3] if len(mp) else None, mocap_quat=mp[:, 3:] if len(mp) else None,
                      time=float(tr.times[2]))


def assert_member_equals_planner(b, p, where):
    """b: a member of the fleet, p: the sequential GpuRobustPlanner"""
    assert b.delegate.trajectory_order == p.delegate.trajectory_order, where
    assert b.delegate._scores == p.delegate._scores, where
    assert b.best_candidate == p.best_candidate, where
    assert b.perturbed_score == p.perturbed_score and b.valid_rollouts == p.valid_rollouts, where
    assert b.delegate.winner == p.delegate.winner, where
    assert np.array_equal(b.delegate.policy.plan.times(), p.delegate.policy.plan.times()), where
    assert np.array_equal(b.delegate.policy.plan.values(), p.delegate.policy.plan.values()), where


def assert_same_trajectory(tb, ts, where):
    assert tb.total_return == ts.total_return and tb.failure == ts.failure, where
    for k in ("states", "actions", "times", "residual", "costs", "trace"):
        assert np.array_equal(getattr(tb, k), getattr(ts, k)), (where, k)


def run_fleet_against_members(task, k, R, xfrc_std=None, tasks=None, zero=False, steps=STEPS, factory=backend):
    """factory: the contexts' backend (the oracle's here; None: the device's, tests/test_gpu_batch_robust.py)"""
    H = HORIZON[task.name]
    if task.name == "QuadrupedFlat":
        task.transition(0.0)
    batch = fleet_planner(task, k, R, xfrc_std, tasks, factory=factory)
    singles = [single_planner(tasks[e] if tasks is not None else task, SEED + e, k, R, xfrc_std, factory=factory) for e in range(E)]
    batch.reset(H)
    for p in singles:
        p.reset(H)
    states = initial_states(task, zero)
    valid = []
    for step in range(steps):
        batch.set_states(states)
        batch.optimize_policy(H)
        for e, p in enumerate(singles):
            p.set_state(states[e])
            p.optimize_policy(H)
            assert len(p.delegate.trajectory_order) == k and len(p.perturbed_score) == k
            assert p.iteration == step + 1 == batch.envs[e].iteration     # the noise offset advances with the iteration
            assert_member_equals_planner(batch.envs[e], p, (step, e))
            assert_same_trajectory(batch.best_trajectory(e), p.best_trajectory(), (step, e))
            x, y = np.zeros(task.model.nu), np.zeros(task.model.nu)
            batch.action_from_policy(e, x, None, states[e].time + 0.005)
            p.action_from_policy(y, None, states[e].time + 0.005)
            assert np.array_equal(x, y)
            valid.append((list(p.valid_rollouts), list(p.perturbed_score), list(p.delegate._scores)))
        step_along(task, states, singles)
    return batch, singles, valid


@pytest.mark.parametrize("k,R", PAIRS)
@pytest.mark.parametrize("name", ["Cartpole", "Particle", "QuadrupedFlat"])
def test_fleet_is_one_robust_planner_per_environment(name, k, R):
    task = load_task(name)
    batch, singles, valid = run_fleet_against_members(task, k, R)
    # the perturbation changed something: some rank's score is not its unperturbed return, and the environments are different problems
    assert any(score != ret for _, scores, rets in valid for score, ret in zip(scores, rets))
    assert len({tuple(np.round(p.delegate.policy.plan.values().ravel(), 12)) for p in batch.envs}) == E
    # the second context's last rollout is the padded noisy one
    assert batch.ctx.n_per_env == 64 * ((k * R + 63) // 64) and batch.ctx.N == E * batch.ctx.n_per_env


def test_one_candidate_takes_the_delegates_ordinary_step(cartpole):
    batch, singles, _ = run_fleet_against_members_k1(cartpole)
    assert all(p.best_candidate == 0 for p in batch.envs) and batch.iteration == 0 and batch.ctx.N == 0   # no perturbed launch at all


def run_fleet_against_members_k1(task):
    H = HORIZON[task.name]
    batch = fleet_planner(task, 1, 4)
    singles = [single_planner(task, SEED + e, 1, 4) for e in range(E)]
    batch.reset(H)
    for p in singles:
        p.reset(H)
    states = initial_states(task)
    for step in range(STEPS):
        batch.set_states(states)
        batch.optimize_policy(H)
        for e, p in enumerate(singles):
            b = batch.envs[e]
            p.set_state(states[e])
            p.optimize_policy(H)
            assert b.delegate.trajectory_order == p.delegate.trajectory_order and b.delegate._scores == p.delegate._scores, (step, e)
            assert b.best_candidate == p.best_candidate == 0 and p.iteration == 0
            assert np.array_equal(b.delegate.policy.plan.times(), p.delegate.policy.plan.times()), (step, e)
            assert np.array_equal(b.delegate.policy.plan.values(), p.delegate.policy.plan.values()), (step, e)
            assert_same_trajectory(batch.best_trajectory(e), p.best_trajectory(), (step, e))
        step_along(task, states, singles)
    return batch, singles, None


@pytest.mark.parametrize("name", ["Particle", "QuadrupedFlat"])
def test_fleet_with_tasks_is_one_robust_planner_per_task(name):
    """set_tasks: every robot its own weights, norm parameters, parameters and risk (the A1s their own gait and mode as well), on BOTH contexts"""
    task = load_task(name)
    if name == "QuadrupedFlat":
        task.transition(0.0)
    tasks = task_rows.unlike_tasks(task, E)
    batch, singles, _ = run_fleet_against_members(task, 5, 4, tasks=tasks, steps=2)
    want = task_rows.rows_of(tasks)
    for ctx in (batch.ctx, batch.delegate.ctx):
        push = ctx.pushes[-1]
        for key in ("weight", "norm_parameter", "parameters"):
            assert np.array_equal(push[key].reshape(want[key].shape), want[key]), key
    # the rows decide the cost: the same candidate order would be a coincidence
    assert len({tuple(p.perturbed_score) for p in batch.envs}) == E


# force noise at which only SOME perturbed Particle rollouts fail (below 1e9 none does, above 3e9 nearly all do). Found with the oracle on
# particle_failure_scenario below: of the 15 (environment, rank) pairs, 1.4e9 leaves 6 with all four repetitions valid and 9 with some,
# 2.3e9 leaves 7 with some and 8 with none
FAILURE_STD = (1.4e9, 2.3e9)


def test_failed_perturbed_rollouts_do_not_count(particle):
    """Particle under a force noise so large that mj_checkAcc stops some perturbed rollouts: per (environment, rank) the sequential
    planners' own flags show every case -- some repetitions valid, none (the score is then the unperturbed return, bit for bit), all --
    and the fleet equals them in each."""
    cases = set()
    for std in FAILURE_STD:
        _, singles, valid = run_fleet_against_members(particle, 5, 4, xfrc_std=std, zero=True)
        for counts, scores, rets in valid:
            for c, score, ret in zip(counts, scores, rets):
                cases.add("none" if c == 0 else "all" if c == 4 else "some")
                if c == 0:
                    assert score == ret
    assert cases == {"none", "some", "all"}, cases


def particle_failure_scenario():
    """the Particle at rest at the origin, three goals, 64 random splines per environment"""
    task = load_task("Particle")
    rng = np.random.default_rng(23)
    m = task.model
    dt = m.get_number("agent_timestep", m.timestep)
    Hf, Pf = 12, 4
    states = np.zeros((E, m.nq + m.nv))
    mocap = np.array([[0.1 * (e + 1), -0.05 * e, 0.01, 1, 0, 0, 0] for e in range(E)], float)
    times = np.stack([np.arange(Pf) * ((Hf - 1) * dt / (Pf - 1))] * E)
    values = np.clip(rng.normal(0, 0.5, (E, 64, Pf, m.nu)), -1, 1)
    return task, Hf, states, mocap, times, values


def failure_mix(make_context, stds=FAILURE_STD):
    """-> the cases ("none", "some", "all" of a rank's repetitions valid) the sequential side's own flags show, asserting the device call
    against it at every force noise"""
    task, Hf, states, mocap, times, values = particle_failure_scenario()
    k, R, cases = 5, 4, {}
    src, ctx = make_context(task), make_context(task)
    for c in (src, ctx):
        c.set_states(states, np.zeros(E), mocap)
    src.rollout_splines_batched(Hf, capi.SPLINE_CUBIC, times, values, num_envs=E, n_per_env=64)
    for std in stds:
        dev = ctx.robust_step_batched(src, E, k, R, Hf, capi.SPLINE_CUBIC, times, std, 0.1, seed=9, candidate_offset=0)
        dev["returns"], dev["failure"] = ctx.returns()
        n, n_pad = 64, 64
        idx, cret = src.ce_update_batched(E, k, -1)[:2]
        chosen = np.stack([[src.fetch_spline(e * n + int(i)) for i in idx[e]] for e in range(E)])
        ctx.rollout_splines_noisy_batched(Hf, capi.SPLINE_CUBIC, times, chosen[:, np.minimum(np.arange(n_pad) // R, k - 1)], std, 0.1, seed=9, candidate_offset=0,
                                          num_envs=E, n_per_env=n_pad)
        ret, fail = ctx.returns()
        assert np.array_equal(ret, dev["returns"], equal_nan=True) and np.array_equal(fail, dev["failure"])
        for e in range(E):
            sl = slice(e * n_pad, e * n_pad + k * R)
            scores, valid, best = robust_scores(cret[e], ret[sl], fail[sl], R)
            assert np.array_equal(dev["perturbed_score"][e], scores, equal_nan=True) and dev["valid"][e].tolist() == valid and dev["best"][e] == best
            assert np.array_equal(dev["candidate"][e], idx[e]) and np.array_equal(dev["candidate_return"][e], cret[e])
            for c, v in enumerate(valid):
                kind = "none" if v == 0 else "all" if v == R else "some"
                cases[kind] = cases.get(kind, 0) + 1
                if v == 0:
                    assert dev["perturbed_score"][e][c] == cret[e][c]     # no valid repetition: the unperturbed return, bit for bit
    return cases


def test_failed_perturbed_rollouts_in_one_robust_step():
    """robust_step_batched itself on that scenario (the device runs the same one, tests/test_gpu_batch_robust.py): every case shows"""
    cases = failure_mix(backend)
    assert set(cases) == {"none", "some", "all"} and min(cases.values()) >= 2, cases


def test_the_running_mean_is_the_planners():
    """robust_scores, the loop of RobustPlanner::OptimizePolicy: the order of operations, failed rollouts, ties and NaN"""
    ret = np.array([1.0, 2.0, 4.0, 0.5, 0.5, 0.5, 9.0, 9.0, 9.0])
    fail = np.array([0, 1, 0, 0, 0, 0, 1, 1, 1])
    scores, valid, best = robust_scores([3.0, 0.5, 0.25], ret, fail, 3)
    assert scores == [(1 * ((0 * 3.0 + 1.0) / 1) + 4.0) / 2, 0.5, 0.25] and valid == [2, 3, 0] and best == 2
    assert robust_scores([1.0, 1.0], [1.0, 1.0], [0, 0], 1)[2] == 0                       # a tie: the lower rank
    assert robust_scores([1.0, float("nan")], [1.0, 0.0], [0, 1], 1)[2] == 0               # a NaN never beats an earlier rank
    assert robust_scores([float("nan"), 1.0], [0.0, 1.0], [1, 0], 1)[2] == 0               # ... and nothing beats a NaN at rank 0 (strict <)
    x = robust_scores([0.1], [0.2, 0.3, 0.7], [0, 0, 0], 3)[0][0]
    assert x == (2 * ((1 * ((0 * 0.1 + 0.2) / 1) + 0.3) / 2) + 0.7) / 3


def test_a_sharded_delegate_is_refused():
    class Group:
        rank, world = 0, 2
    with pytest.raises(ValueError, match="one rank"):
        GpuRobustPlanner(GpuSamplingPlanner(group=Group()))


def test_settings_as_initialize_reads_them(cartpole):
    p = GpuRobustPlanner(GpuSamplingPlanner())
    p.initialize(cartpole.model, cartpole)
    m = cartpole.model
    R = int(m.get_number("robust_repetitions", 5))
    assert p.nrepetitions_ == R and p.xfrc_std_ == m.get_number("robust_xfrc", 0.1) and p.xfrc_rate_ == m.get_number("robust_xfrc_rate", 0.1)
    want = int(m.get_number("robust_candidates", -1))
    assert p.ncandidates_ == (want if want != -1 else int(m.get_number("sampling_trajectories", 10)) // max(R, 1))
    fleet = GpuBatchRobustPlanner(2)
    fleet.initialize(m, cartpole)
    fleet.ncandidates_, fleet.xfrc_std_ = 7, 0.25
    assert all((q.ncandidates_, q.xfrc_std_) == (7, 0.25) for q in fleet.envs) and isinstance(fleet.delegate, GpuBatchSamplingPlanner)
