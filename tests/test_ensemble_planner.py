"""GpuEnsembleSamplingPlanner (one robot, M hypotheses, one set of candidates) without a device, on tests/ensemble_oracle_backend.py.

   one hypothesis, any tail, and four identical hypotheses at tail 1 and 4: the plan of GpuSamplingPlanner(seed), bit for bit, over three
       plan steps -- policy, winner, returns, actions (the mean of equal doubles is exact)
   three unlike models (base, payload, ice): every hypothesis rolls out the same splines; the winner and its score are the argmin of the
       score recomputed here from three SINGLE oracle rollouts with the same seed, by the definition written as a plain loop
   CASE, the case the device tests reuse: the ensemble's winner is not hypothesis 0's own argmin, and the best score is clear of the second
       best by more than 100 x the device tests' parity bound -- so a selection that returned best_batched(...)[0] would be told apart, and
       an index disagreement there would not be noise
   the length checks of set_models / set_tasks / set_states, and tail outside 1..M"""
import numpy as np
import pytest

import model_variants as mv
import task_rows
import test_batch_models as cpu
import test_batch_robust_planner as tr
from ensemble_oracle_backend import EnsembleOracleContext, ensemble_argmin, ensemble_scores
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import GpuEnsembleSamplingPlanner, GpuSamplingPlanner, State
from oracle_backend import OracleContext

T, STD = 6, 0.05
# the planner case of the device tests (tests/test_gpu_ensemble.py): A1, three hypotheses -- the models base / payload / ice, each with a task
# row of its own (task_rows.unlike_tasks: other weights, gait and mode) -- n x H, the mean score. With the models alone hypothesis 0's own
# argmin won under every seed tried (over H = 6 the returns of the three models rank the candidates alike). The seed was chosen on the
# oracle, among 0..19, for the two properties test_the_case_tells_the_score_from_hypothesis_0 asserts, in both plan steps
CASE = dict(robot="a1", unlike_tasks=True, std=STD, seed=18, n=1024, horizon=6, tail=3, steps=2)
QUAD_BOUND = 1e-9          # tests/test_gpu_batch.py's bound of the quad kernel: 1e-9 (1 + |x|)
# the same for the limb kernel in fp32, whose returns are held to 2e-3 (1 + |x|): the Humanoid of tests/model_variants.py, base / payload /
# ice with unlike task rows. A device score within the bound b of the oracle's keeps the oracle's argmin when the oracle's best score is
# clear of its second best by more than 2 b (the best may rise by b, the second best fall by b) -- that is the gap this case must have;
# 100 b, what CASE has of its bound, would be a fifth of the score itself and no set of candidates has it. At the launch tests' 1280 x 4 the
# best scores lie 0.3 b apart; 64 candidates of exploration 0.1 over H = 16 do spread: chosen on the oracle among n in {64, 128, 256},
# exploration in {0.05, 0.1, 0.15}, H in {4, 8, 16} and seeds 0..9 for the widest gap in both plan steps with a winner that is neither the
# nominal nor hypothesis 0's own argmin
LIMB_CASE = dict(robot="humanoid", unlike_tasks=True, std=0.1, seed=3, n=64, horizon=16, tail=3, steps=2)
LIMB32_BOUND = 2e-3


def oracle_factory(t):
    return EnsembleOracleContext(t, threads=8)


def ensemble(task, M, seed, tail, n=64, factory=oracle_factory, precision=64):
    p = GpuEnsembleSamplingPlanner(M, seed=seed, tail=tail, backend_factory=factory, precision=precision)
    p.initialize(task.model, task)
    p.num_trajectory_ = n
    p.noise_exploration = [STD, 0.0]
    p.allocate()
    return p


def single(task, seed, n=64, factory=lambda t: OracleContext(t, threads=8)):
    p = GpuSamplingPlanner(seed=seed, backend_factory=factory)
    p.initialize(task.model, task)
    p.num_trajectory_ = n
    p.noise_exploration = [STD, 0.0]
    p.allocate()
    return p


def a1():
    task, models, tasks = cpu.fleet_models()
    return task, models, tasks, tr.initial_states(task)[0]


def advance(task, state, trajectory):
    nq = task.model.nq
    mp = state.mocap.reshape(-1, 7)
    state.set(trajectory.states[2, :nq], trajectory.states[2, nq:], mocap_pos=mp[:, :3] if len(mp) else None,
              mocap_quat=mp[:, 3:] if len(mp) else None, time=float(trajectory.times[2]))


@pytest.mark.parametrize("M,tail", [(1, None), (1, 1), (4, 1), (4, 4)])
def test_alike_hypotheses_plan_like_the_single_planner(M, tail):
    task, models, tasks, state = a1()
    ens, one = ensemble(task, M, 5, tail), single(task, 5)
    ens.reset(T)
    one.reset(T)
    for step in range(3):
        ens.set_state(state)
        one.set_state(state)
        ens.optimize_policy(T)
        one.optimize_policy(T)
        where = (M, tail, step)
        assert ens.winner == one.winner and ens.iteration == one.iteration, where
        assert (ens.best_score, ens.nominal_score, ens.improvement) == (one.best_return, one.nominal_return, one.improvement), where
        assert np.array_equal(ens.member_returns, np.full(M, one.best_return)), where
        assert np.array_equal(ens.policy.plan.times(), one.policy.plan.times()) and np.array_equal(ens.policy.plan.values(), one.policy.plan.values()), where
        for h in range(M):
            tr.assert_same_trajectory(ens.best_trajectory(h), one.best_trajectory(), where)
        for t in (state.time, state.time + 0.013, state.time + 0.04):
            assert np.array_equal(ens.action_from_policy(np.zeros(task.model.nu), None, t), one.action_from_policy(np.zeros(task.model.nu), None, t)), where
        advance(task, state, one.best_trajectory())


def single_rollouts(tasks, state, ens, n, horizon, seed, iteration, times, values):
    """M x n returns and the n splines from M SINGLE oracle rollouts (a context per model) with the same seed"""
    ns = capi.make_noise_spec(seed=seed, iteration=iteration, mode=capi.NOISE_SAMPLING, candidate_offset=0, nominal_candidate=0, std0=STD, std1=0.0)
    rows, splines = [], []
    for t in tasks:
        ctx = OracleContext(t, threads=8)
        ctx.set_state(state.state, state.time, state.mocap)
        ctx.rollout_noise(n, horizon, ens.policy.plan.interpolation(), times, values, ns)
        rows.append(ctx.returns()[0])
        splines.append(ctx.nodes.copy())
    return np.stack(rows), splines


@pytest.mark.parametrize("tail", [1, 2, 3])
def test_unlike_models_share_the_candidates_and_the_winner_is_the_scores_argmin(tail):
    task, models, tasks, state = a1()
    M, n = 3, 64
    ens = ensemble(task, M, 11, tail)
    ens.set_models(models)
    ens.reset(T)
    launches, launch = [], ens.ctx.rollout_noise_ensemble

    def recorded(n_, horizon, interp, node_times, nominal, ns, num_hypotheses):        # the nominal the plan step resampled
        launches.append((np.array(node_times, float), np.array(nominal, float)))
        return launch(n_, horizon, interp, node_times, nominal, ns, num_hypotheses)
    ens.ctx.rollout_noise_ensemble = recorded
    for step in range(2):
        ens.set_state(state)
        ens.optimize_policy(T)
        times, values = launches[-1]
        for i in (0, 1, n // 2, n - 1, ens.winner):
            for h in range(1, M):
                assert np.array_equal(ens.ctx.fetch_spline(h * n + i), ens.ctx.fetch_spline(i)), (step, h, i)
        R, splines = single_rollouts(tasks, state, ens, n, T, 11, step, times, values)
        for h in range(M):
            assert np.array_equal(splines[h], splines[0]) and np.array_equal(ens.ctx.returns()[0][h * n:(h + 1) * n], R[h]), (step, h)
        assert len({float(R[h, 0]) for h in range(M)}) == M          # (the models decide the cost)
        scores = ensemble_scores(R, tail)
        w = ensemble_argmin(scores)
        assert ens.winner == w and ens.best_score == scores[w] and ens.nominal_score == scores[0], (step, tail)
        assert np.array_equal(ens.member_returns, R[:, w]), (step, tail)
        assert np.array_equal(ens.policy.plan.values(), splines[0][w]), (step, tail)
        for h in range(M):
            assert ens.best_trajectory(h).total_return == R[h, w], (step, h)
        advance(task, state, ens.best_trajectory())


def humanoid():
    """the Humanoid of tests/model_variants.py: its task with the bank state's frozen residual state, base / payload / ice, that state"""
    r = mv.robot("humanoid")
    s = r.state
    task = task_rows.copy_task(r.task)
    task.residual_int, task.residual_real = list(s.residual_int), list(s.residual_real)
    state = State(task.model)
    mocap = np.asarray(s.mocap, float).reshape(-1, 7)
    nq = task.model.nq
    state.set(s.state[:nq], s.state[nq:], mocap_pos=mocap[:, :3], mocap_quat=mocap[:, 3:], time=s.time)
    return task, [r.base, r.mixed["payload"], r.mixed["ice"]], None, state


def run_case(factory=oracle_factory, precision=64, case=None):
    """the planner of a case (CASE, LIMB_CASE) over its plan steps; per step the winner, best_score, nominal_score, member_returns, every
    score, hypothesis 0's returns and the winner's trajectory under hypothesis 0, from which the next step starts"""
    case = CASE if case is None else case
    task, models, tasks, state = humanoid() if case["robot"] == "humanoid" else a1()
    M = len(models)
    ens = GpuEnsembleSamplingPlanner(M, seed=case["seed"], tail=case["tail"], backend_factory=factory, precision=precision)
    ens.initialize(task.model, task)
    ens.num_trajectory_ = case["n"]
    ens.noise_exploration = [case["std"], 0.0]
    ens.allocate()
    ens.set_models(models)
    if case["unlike_tasks"]:
        ens.set_tasks(task_rows.unlike_tasks(task, M))
    ens.reset(case["horizon"])
    out = []
    for step in range(case["steps"]):
        ens.set_state(state)
        ens.optimize_policy(case["horizon"])
        scores = ens.ctx.ensemble_best(M, case["tail"], 0, with_scores=True)[5]
        out.append(dict(winner=ens.winner, best_score=ens.best_score, nominal_score=ens.nominal_score, member_returns=ens.member_returns.copy(),
                        scores=np.array(scores), returns0=ens.ctx.returns()[0][:case["n"]].copy(), trajectory=ens.best_trajectory()))
        advance(task, state, out[-1]["trajectory"])
    return ens, out


_ON_THE_ORACLE = {}


def case_on_the_oracle(case=None):
    """computed once per case, shared with the device tests, left unchanged"""
    case = CASE if case is None else case
    key = tuple(sorted(case.items()))
    if key not in _ON_THE_ORACLE:
        _ON_THE_ORACLE[key] = run_case(case=case)[1]
    return _ON_THE_ORACLE[key]


def test_the_case_tells_the_score_from_hypothesis_0():
    for step, got in enumerate(case_on_the_oracle()):
        scores, w = got["scores"], got["winner"]
        assert w == ensemble_argmin(scores)
        own = int(np.lexsort((np.arange(len(got["returns0"])), got["returns0"]))[0])
        assert w != own, (step, "the ensemble's winner is hypothesis 0's own argmin: best_batched(...)[0] would pass for the score")
        second = np.partition(scores, 1)[1]
        gap = second - scores[w]
        print(f"step {step}: winner {w} (hypothesis 0's own argmin: {own}), best score {scores[w]!r}, second best {second!r}, gap {gap:.3e}")
        assert gap > 100 * QUAD_BOUND * (1 + abs(scores[w])), (step, gap)


def test_the_limb_case_has_a_gap_that_fp32_resolves():
    for step, got in enumerate(case_on_the_oracle(LIMB_CASE)):
        scores, w = got["scores"], got["winner"]
        assert w == ensemble_argmin(scores) and w != 0
        own = int(np.lexsort((np.arange(len(got["returns0"])), got["returns0"]))[0])
        assert w != own, (step, "the ensemble's winner is hypothesis 0's own argmin")
        second = np.partition(scores, 1)[1]
        bound = LIMB32_BOUND * (1 + abs(scores[w]))
        print(f"step {step}: winner {w} (hypothesis 0's own argmin: {own}), best score {scores[w]!r}, second best {second!r}, gap {second - scores[w]:.3e} = "
              f"{(second - scores[w]) / bound:.2f} x the bound")
        assert second - scores[w] > 2 * bound, (step, second - scores[w], bound)


def test_length_checks_and_tail():
    task, models, tasks, state = a1()
    for tail in (0, 4, -1):
        with pytest.raises(ValueError, match="tail"):
            GpuEnsembleSamplingPlanner(3, tail=tail)
    with pytest.raises(ValueError, match="at least one"):
        GpuEnsembleSamplingPlanner(0)
    with pytest.raises(ValueError, match="at most 32"):
        GpuEnsembleSamplingPlanner(33)
    ens = ensemble(task, 3, 0, None)
    assert ens.tail == 3
    assert not hasattr(ens, "winners") and ens.winner == 0          # one robot: the fleet's list of winners is hidden
    with pytest.raises(ValueError, match="2 models for 3 environments"):
        ens.set_models(models[:2])
    with pytest.raises(ValueError, match="2 tasks for 3 environments"):
        ens.set_tasks(tasks[:2])
    with pytest.raises(ValueError, match="2 states for 3 environments"):
        ens.set_states([state, state])
    ens.num_trajectory_ = 100
    ens.reset(T)
    ens.set_state(state)
    with pytest.raises(ValueError, match="multiple of 64"):
        ens.optimize_policy(T)
    with pytest.raises(ValueError, match="hypothesis 3"):
        ens.best_trajectory(3)


def test_hypotheses_about_the_task_and_the_state():
    """set_tasks and set_states: a hypothesis's own task row and state reach its rollouts (the returns of the shared nominal differ)"""
    task, models, tasks, state = a1()
    rows = task_rows.unlike_rows(task, 3)
    unlike = []
    for e in range(3):
        t = task_rows.copy_task(task)
        t.weight = [float(x) for x in rows["weight"][e]]
        unlike.append(t)
    ens = ensemble(task, 3, 2, 1)
    ens.reset(T)
    ens.set_tasks(unlike)
    ens.set_state(state)
    ens.optimize_policy(T)
    r = ens.ctx.returns()[0].reshape(3, -1)
    assert len({float(x) for x in r[:, 0]}) == 3
    assert ens.best_score == max(ens.member_returns)             # (tail 1: the worst case)
    ens.set_tasks(None)
    ens.set_states(tr.initial_states(task))
    ens.optimize_policy(T)
    r = ens.ctx.returns()[0].reshape(3, -1)
    assert len({float(x) for x in r[:, 0]}) == 3
    for i in (0, 7, 63):
        assert np.array_equal(ens.ctx.fetch_spline(64 + i), ens.ctx.fetch_spline(i))
