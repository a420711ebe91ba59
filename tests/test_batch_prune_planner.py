"""Pruning and parking for a fleet, off the device: the two C symbols (mjpcx_set_pruning_batched, mjpcx_prune_stats_batched) are declared,
exported and bound, and GpuBatchSamplingPlanner(pruning=True) on a stand-in backend that really retires candidates
(tests/batch_prune_oracle_backend.py) plans exactly like E single GpuSamplingPlanners, passes the hints the C++ planner's rules give,
repeats a refused launch unpruned and keeps the switch off for everything else."""
import os
import re

import numpy as np
import pytest

from batch_prune_oracle_backend import PRUNED, BatchPruneOracleContext
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import GpuBatchSamplingPlanner, GpuSamplingPlanner, State, cost_is_non_negative, task_signature
from oracle_backend import OracleContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, N_PER_ENV, STEPS, SEED = 3, 64, 3, 5


def test_the_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mjpcx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, method in (("mjpcx_set_pruning_batched", "set_pruning_batched"), ("mjpcx_prune_stats_batched", "prune_stats_batched")):
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert name in capi.EXPORTS
        assert hasattr(capi.lib(), name) and getattr(capi.lib(), name).argtypes is not None
        assert callable(getattr(capi.Context, method))
    # the header comment of mjpcx_set_pruning points to the new call
    doc = text[:text.index("int mjpcx_set_pruning(")]
    assert "mjpcx_set_pruning_batched" in doc[doc.rindex("/*"):]


def batch_planner(task, pruning=True, **kw):
    p = GpuBatchSamplingPlanner(E, seed=SEED, backend_factory=lambda t: BatchPruneOracleContext(t, **kw))
    p.initialize(task.model, task)
    p.num_trajectory_ = N_PER_ENV
    p.allocate()
    p.pruning = pruning
    return p


def single_planner(task, seed):
    p = GpuSamplingPlanner(seed=seed, backend_factory=lambda t: OracleContext(t))
    p.initialize(task.model, task)
    p.num_trajectory_ = N_PER_ENV
    p.allocate()
    return p


def initial_states(task):
    m = task.model
    rng = np.random.default_rng(17)
    out = []
    for e in range(E):
        st = State(m)
        q, v = rng.uniform(-0.5, 0.5, m.nq) * (0.2 if m.nmocap else 1.0), rng.normal(0, 0.3, m.nv)
        if m.nmocap:
            st.set(q, v, mocap_pos=[[0.1 * (e + 1), -0.05 * e, 0.01]], mocap_quat=[[1, 0, 0, 0]], time=0.1 * e)
        else:
            st.set(q, v, time=0.1 * e)
        out.append(st)
    return out


def advance(task, states, trajectories):
    nq = task.model.nq
    for e, tr in enumerate(trajectories):
        mp = states[e].mocap.reshape(-1, 7)
        states[e].set(tr.states[2, :nq], tr.states[2, nq:], mocap_pos=mp[:, :3] if len(mp) else None, mocap_quat=mp[:, 3:] if len(mp) else None,
                      time=float(tr.times[2]))


HORIZON = 30


@pytest.fixture
def task(cartpole):
    """Cartpole: smooth-abs and quadratic terms with weights >= 0 and no risk transform, so the planner may prune (Particle's risk is 1)"""
    assert cost_is_non_negative(cartpole)
    return cartpole


def test_default_is_off_and_the_slack_is_the_c_planners(task):
    p = batch_planner(task, pruning=False)
    fresh = GpuBatchSamplingPlanner(E)
    assert fresh.pruning is False and fresh.park_slack == 0.05 and p.park_slack == 0.05


def test_a_pruned_fleet_plans_like_one_sampling_planner_per_environment(task):
    H = HORIZON
    batch, singles = batch_planner(task), [single_planner(task, SEED + e) for e in range(E)]
    batch.reset(H)
    for p in singles:
        p.reset(H)
    states = initial_states(task)
    for step in range(STEPS):
        batch.set_states(states)
        batch.optimize_policy(H)
        log = batch.ctx.launches[-1]
        assert log["pruned"] and (log["retired"] > 0).all() and batch.ctx.switch is None     # really pruned, and the switch cleared after the launch
        assert np.array_equal(batch.prune_stats["retired"], log["retired"]) and (batch.park_stats["resumed"] == 0).all()
        assert not batch.pruned_launch_repeated
        ret, fail = batch.ctx.returns()
        assert ((fail & PRUNED) != 0).sum() == log["retired"].sum()
        for e, p in enumerate(singles):
            p.set_state(states[e])
            p.optimize_policy(H)
            assert batch.winners[e] == p.winner, (step, e)
            assert np.array_equal(batch.envs[e].policy.plan.times(), p.policy.plan.times()), (step, e)
            assert np.array_equal(batch.envs[e].policy.plan.values(), p.policy.plan.values()), (step, e)
            assert batch.envs[e].best_return == p.best_return and batch.envs[e].nominal_return == p.nominal_return
            assert batch.envs[e].improvement == p.improvement
            tb, ts = batch.best_trajectory(e), p.best_trajectory()
            for k in ("states", "actions", "times", "costs"):
                assert np.array_equal(getattr(tb, k), getattr(ts, k)), (step, e, k)
            assert tb.total_return == ts.total_return
            # the hint rules: none on the first plan, then the robot's previous best x 1.05
            if step == 0:
                assert np.isinf(log["hints"][e])
            else:
                assert log["hints"][e] == previous_best[e] * (1.0 + 0.05)
        previous_best = [p.best_return for p in singles]
        advance(task, states, [p.best_trajectory() for p in singles])
    assert len({tuple(np.round(p.policy.plan.values().ravel(), 12)) for p in singles}) == E


def test_hints_are_dropped_after_a_task_row_edit_and_after_a_stale_plan(task):
    import copy
    H = HORIZON
    batch = batch_planner(task)
    tasks = [copy.deepcopy(task) for _ in range(E)]
    batch.set_tasks(tasks)
    batch.reset(H)
    states = initial_states(task)
    hints = []
    for step in range(5):
        if step == 2:
            tasks[1].weight[0] *= 4.0                       # robot 1's task row changes before plan 2
        if step == 3:
            batch.ctx.resume_next = [0, 0, N_PER_ENV // 4 + 1]   # plan 3 resumes more than a quarter of robot 2's candidates ...
        batch.set_states(states)
        batch.optimize_policy(H)
        hints.append(batch.ctx.launches[-1]["hints"])
        assert np.array_equal(hints[-1], batch.park_hints_used)
        best = [p.best_return for p in batch.envs]
        advance(task, states, [batch.best_trajectory(e) for e in range(E)])
        if step == 0:
            first_best = best
    # (the backend applies the rows: from plan 2 on robot 1 really rolls out on its edited weights)
    w = [push["weight"] for push in batch.ctx.pushes]
    assert w[1][1, 0] == w[0][1, 0] and w[2][1, 0] == 4.0 * w[0][1, 0] and np.array_equal(w[2][0], w[0][0])
    assert np.isinf(hints[0]).all()
    assert np.array_equal(hints[1], np.array(first_best) * 1.05)
    assert np.isfinite(hints[2][0]) and np.isinf(hints[2][1]) and np.isfinite(hints[2][2])
    assert np.isfinite(hints[3]).all()                      # (the edited row is the row the hint of plan 2 was taken under)
    assert np.isfinite(hints[4][0]) and np.isfinite(hints[4][1]) and np.isinf(hints[4][2])   # ... so robot 2 plans without a hint next
    assert (batch.ctx.launches[3]["hints"] >= 0).all()
    # exactly a quarter is not stale
    batch.ctx.resume_next = [N_PER_ENV // 4, 0, 0]
    batch.set_states(states)
    batch.optimize_policy(H)
    batch.set_states(states)
    batch.optimize_policy(H)
    assert np.isfinite(batch.ctx.launches[-1]["hints"]).all()
    # a slack of -1 or less: no hints at all
    batch.park_slack = -1.0
    batch.set_states(states)
    batch.optimize_policy(H)
    assert np.isinf(batch.ctx.launches[-1]["hints"]).all() and batch.ctx.launches[-1]["pruned"]


def test_a_refused_argmin_is_repeated_unpruned_with_the_same_seed_and_iteration(task):
    H = HORIZON
    batch, ref = batch_planner(task), batch_planner(task, pruning=False)
    states = initial_states(task)
    for p in (batch, ref):
        p.reset(H)
        p.set_states(states)
    batch.ctx.refuse_next_best = True
    batch.optimize_policy(H)
    ref.optimize_policy(H)
    a, b = batch.ctx.launches[-2:]
    assert a["pruned"] and not b["pruned"] and b["kind"] == "noise" and (a["seed"], a["iteration"]) == (b["seed"], b["iteration"])
    assert batch.pruned_launch_repeated and len(batch.ctx.launches) == 2 and batch.iteration == ref.iteration == 1
    _, fail = batch.ctx.returns()
    assert not (fail & PRUNED).any()
    for e in range(E):
        assert batch.winners[e] == ref.winners[e] and batch.envs[e].best_return == ref.envs[e].best_return
        assert np.array_equal(batch.envs[e].policy.plan.values(), ref.envs[e].policy.plan.values())
    # any other error is not swallowed
    class Boom(BatchPruneOracleContext):
        def best_batched(self, *a, **kw):
            raise ValueError("boom")
    p = GpuBatchSamplingPlanner(E, seed=SEED, backend_factory=lambda t: Boom(t))
    p.initialize(task.model, task)
    p.num_trajectory_ = N_PER_ENV
    p.allocate()
    p.pruning = True
    p.reset(H)
    p.set_states(states)
    with pytest.raises(ValueError):
        p.optimize_policy(H)
    assert p.ctx.switch is None and len(p.ctx.launches) == 1


def test_nominal_trajectory_and_an_unpruned_planner_keep_the_switch_off(task):
    H = HORIZON
    batch = batch_planner(task)
    batch.reset(H)
    batch.set_states(initial_states(task))
    batch.optimize_policy(H)
    batch.nominal_trajectory(H)
    assert [(l["kind"], l["switch_on"]) for l in batch.ctx.launches] == [("noise", True), ("splines", False)]
    off = batch_planner(task, pruning=False)
    off.reset(H)
    off.set_states(initial_states(task))
    off.optimize_policy(H)
    assert [(l["kind"], l["switch_on"]) for l in off.ctx.launches] == [("noise", False)]
    assert off.prune_stats is None and off.park_stats is None and off.park_hints_used is None


def test_a_cost_that_can_be_negative_in_one_task_row_turns_pruning_off_for_the_launch(task):
    import copy
    H = HORIZON
    batch = batch_planner(task)
    tasks = [copy.deepcopy(task) for _ in range(E)]
    tasks[2].risk = 0.5
    assert not cost_is_non_negative(tasks[2]) and task_signature(tasks[2]) != task_signature(tasks[0])
    batch.set_tasks(tasks)
    batch.reset(H)
    batch.set_states(initial_states(task))
    batch.optimize_policy(H)
    assert [l["switch_on"] for l in batch.ctx.launches] == [False] and batch.prune_stats is None
